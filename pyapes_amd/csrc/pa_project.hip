// pa_project.hip -- the three streaming kernels of the pressure projection (DESIGN.md section 4 "Projection") and their entry
// points: pa_divergence, the collocated central divergence of a vector field in one pass; pa_project_correct, the gradient
// correction of every component in one launch followed by the ordered BC fill per component; and pa_project_update, the
// correction by the increment phi together with the pressure update of the incremental forms ("Incremental form").
//
// The arithmetic is a definition of this library (the reference has no counterpart).  Per active internal axis a, every
// operation rounded on its own in the grid dtype (no FMA), h_a = 0.5 / dx_a formed in double on the host and converted once:
//   divergence   d = U_a[+1]_a - U_a[-1]_a;  d = d * h_a;  s = s + d   (s starts at +0, axes ascending);   out = scale * s
//   correction   g = p[+1]_c - p[-1]_c;  g = g * h_c;  g = scale * g;  out_c = U_c - g
//   update       the correction with phi for p, in place;  q = p + phi;  [t = chi * nrhs;  q = q + t;]  p = q  at every node
// on the interior set (pa_in_S); off it the divergence is +0 and the correction hands U_c on.  Neighbours wrap around like
// every stencil of the library (pa_nbrs), and are read from the BC-filled input: the caller filled it.
//
// One cell per lane, a grid-stride loop under PA_MAX_GRID: the kernels move (d + 1) / (2 d + 1) / (2 d + 3 or 4) arrays and
// compute next to nothing, so there is nothing to tile.  The streams touched once -- the divergence's `out`, the old U of the
// correction, the old p and nrhs of the update -- go past the caches as non-temporal accesses; the neighbour reads of U / p /
// phi are plain loads, which the caches serve.
#include "pa_project.h"

#include <string.h>

template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_divergence(DevGeom G, ProjVec<T> U, T scale, T* __restrict__ out) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < G.ncell;
       idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t i, j, k;
    pa_decode(G, idx, i, j, k);
    T v = (T)0;
    if (pa_in_S(G, i, j, k)) v = scale * proj_div_sum<T>(G, U, i, j, k);
    __builtin_nontemporal_store(v, out + idx);
  }
}

// U.v[a].p: component of internal axis a, read at the cell only; O.o[a]: where it goes
template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_project_correct(DevGeom G, ProjVec<T> U, Vec<T> pv, T scale, ProjOut<T> O) {
  FieldAcc<T> acc{pv};
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < G.ncell;
       idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t i, j, k;
    pa_decode(G, idx, i, j, k);
    const bool in = pa_in_S(G, i, j, k);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (!G.act[a]) continue;
      O.o[a][idx] = proj_corrected<T>(G, U, acc, scale, a, idx, i, j, k, in);
    }
  }
}

// the update of the incremental (pressure-carrying) forms: the correction of the d components by the increment phi, in place,
// and at the same cell -- on and off the interior set --
//   q = p + phi;  nrhs given: t = chi * nrhs; q = q + t;  p = q
// U and p are read and written by the same lane only; phi's neighbours are plain loads, old U, old p and nrhs non-temporal
template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_project_update(DevGeom G, ProjVec<T> U, Vec<T> phiv, T scale, ProjOut<T> O,
                                                              T* __restrict__ p, const T* __restrict__ nrhs, T chi) {
  FieldAcc<T> acc{phiv};
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < G.ncell;
       idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t i, j, k;
    pa_decode(G, idx, i, j, k);
    const bool in = pa_in_S(G, i, j, k);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (!G.act[a]) continue;
      O.o[a][idx] = proj_corrected<T>(G, U, acc, scale, a, idx, i, j, k, in);
    }
    T q = __builtin_nontemporal_load(p + idx);
    q = q + phiv.p[idx];
    if (nrhs) {
      T t = chi * __builtin_nontemporal_load(nrhs + idx);
      q = q + t;
    }
    p[idx] = q;
  }
}

template <typename T>
static int divergence_t(pa_ctx* c, const void* U, double scale, void* out) {
  static int dbg = -1;
  if (proj_dbg(&dbg, 64)) fprintf(stderr, "[pyapes_hip] k_divergence: generic kernel, %lld cells\n", (long long)c->G.ncell);
  hipLaunchKernelGGL(k_divergence<T>, dim3(pa_grid_blocks(c->G.ncell)), dim3(PA_BLOCK), 0, c->stream, c->G, proj_vec<T>(c, U),
                     (T)scale, (T*)out);
  PA_HIP(c, hipGetLastError());
  return PA_OK;
}

// the ordered BC fill of every component with that component's face values in the bound list (types, order and dxf stay:
// pa_momentum_march's mechanism); the list is restored on every way out
template <typename T>
static int fill_components(pa_ctx* c, void* out, int ncomp, const pa_bc_values* bcv) {
  const int sh = 3 - c->ndim;
  const int64_t nc = c->G.ncell;
  HostBC saved[6];
  for (int f = 0; f < 6; ++f) saved[f] = c->bc[f];
  int rc = PA_OK;
  for (int q = 0; q < ncomp && !rc; ++q) {
    for (int f = 0; f < 2 * c->ndim; ++f) { c->bc[f + 2 * sh].value = bcv[q].value[f]; c->bc[f + 2 * sh].vals = bcv[q].vals[f]; }
    rc = pa_bc_apply_auto<T>(c, (T*)out + q * nc, false);
  }
  for (int f = 0; f < 6; ++f) c->bc[f] = saved[f];
  return rc;
}

// the correction of U by the scalar x into `out`; p non-null: the update, p (and nrhs) carried along.  The kernel, then --
// bcv non-null -- the fill
template <typename T>
static int correct_t(pa_ctx* c, const void* U, int ncomp, const void* x, double scale, void* out, void* p, const void* nrhs,
                     double chi, const pa_bc_values* bcv) {
  static int dbg[2] = {-1, -1};
  if (proj_dbg(&dbg[p != nullptr], 64))
    fprintf(stderr, "[pyapes_hip] k_project_%s%s: generic kernel, %lld cells\n", p ? "update" : "correct",
            p ? (nrhs ? " (rotational)" : "") : (out == U ? " (in place)" : ""), (long long)c->G.ncell);
  const dim3 grid(pa_grid_blocks(c->G.ncell)), block(PA_BLOCK);
  const ProjVec<T> Uv = proj_vec<T>(c, U);
  const Vec<T> xv = pa_vec_self<T>(c, (const T*)x);
  if (p)
    hipLaunchKernelGGL(k_project_update<T>, grid, block, 0, c->stream, c->G, Uv, xv, (T)scale, proj_out<T>(c, out), (T*)p,
                       (const T*)nrhs, (T)chi);
  else
    hipLaunchKernelGGL(k_project_correct<T>, grid, block, 0, c->stream, c->G, Uv, xv, (T)scale, proj_out<T>(c, out));
  PA_HIP(c, hipGetLastError());
  return bcv ? fill_components<T>(c, out, ncomp, bcv) : PA_OK;
}

// one scalar buffer of a call and what is said when it lies on a vector buffer or on a scalar buffer named after it
struct ProjScalar {
  const void* p;
  const char* refusal;
};

// the overlap refusals of a correction, stated once: every scalar against the vectors and against the scalars after it, then
// every face array of `bcv` (null: no fill, nothing to check) against everything.  Null buffers are not part of the call.
static int check_overlaps(pa_ctx* c, const char* who, int ncomp, std::initializer_list<const void*> vecs,
                          std::initializer_list<ProjScalar> scalars, const pa_bc_values* bcv) {
  const size_t cbytes = (size_t)c->G.ncell * c->esize, vbytes = cbytes * (size_t)ncomp;
  for (const ProjScalar* s = scalars.begin(); s != scalars.end(); ++s) {
    bool hit = overlaps(s->p, cbytes, vecs, vbytes);
    for (const ProjScalar* t = s + 1; t != scalars.end(); ++t) hit = hit || overlaps(s->p, cbytes, {t->p}, cbytes);
    if (hit) { pa_set_err(c, "%s: %s", who, s->refusal); return PA_E_ARG; }
  }
  const int64_t n[3] = {c->G.n0, c->G.n1, c->G.n2};
  for (int q = 0; bcv && q < ncomp; ++q)
    for (int f = 0; f < 2 * c->ndim; ++f) {
      const void* face = bcv[q].vals[f];
      const size_t fbytes = cbytes / (size_t)n[(f >> 1) + 3 - c->ndim];
      bool hit = overlaps(face, fbytes, vecs, vbytes);
      for (const ProjScalar& s : scalars) hit = hit || overlaps(face, fbytes, {s.p}, cbytes);
      if (hit) { pa_set_err(c, "%s: a BC face array must not overlap a buffer of the call", who); return PA_E_ARG; }
    }
  return PA_OK;
}

extern "C" {

int pa_divergence(pa_ctx* c, const void* U, int ncomp, double scale, void* out) {
  const char* who = "pa_divergence";
  if (int rc = check_projection_call(c, who, ncomp)) return rc;
  if (!U || !out) { pa_set_err(c, "%s: U and out are needed", who); return PA_E_ARG; }
  const size_t cbytes = (size_t)c->G.ncell * c->esize;
  if (overlaps(out, cbytes, {U}, cbytes * (size_t)ncomp)) { pa_set_err(c, "%s: out must not overlap U", who); return PA_E_ARG; }
  PA_HIP(c, hipSetDevice(c->device));
  return c->dtype == PA_F64 ? divergence_t<double>(c, U, scale, out) : divergence_t<float>(c, U, scale, out);
}

int pa_project_correct(pa_ctx* c, void* U, int ncomp, const void* p, double scale, void* out, const pa_bc_values* bcv) {
  const char* who = "pa_project_correct";
  if (int rc = check_projection_call(c, who, ncomp)) return rc;
  if (!U || !p) { pa_set_err(c, "%s: U and p are needed", who); return PA_E_ARG; }
  if (!out) out = U;
  if (int rc = check_overlaps(c, who, ncomp, {U, out}, {{p, "p must not overlap U or out"}}, bcv)) return rc;
  const size_t vbytes = (size_t)c->G.ncell * c->esize * (size_t)ncomp;
  if (out != U && overlaps(out, vbytes, {U}, vbytes)) { pa_set_err(c, "%s: out is U itself (in place) or a buffer of its own", who); return PA_E_ARG; }
  PaRange range_("pyapes projection correction");
  PA_HIP(c, hipSetDevice(c->device));
  return c->dtype == PA_F64 ? correct_t<double>(c, U, ncomp, p, scale, out, nullptr, nullptr, 0.0, bcv)
                            : correct_t<float>(c, U, ncomp, p, scale, out, nullptr, nullptr, 0.0, bcv);
}

int pa_project_update(pa_ctx* c, void* U, int ncomp, const void* phi, double scale, void* p, const void* nrhs, double chi,
                      const pa_bc_values* bcv) {
  const char* who = "pa_project_update";
  if (int rc = check_projection_call(c, who, ncomp)) return rc;
  if (!U || !phi || !p) { pa_set_err(c, "%s: U, phi and p are needed", who); return PA_E_ARG; }
  if (int rc = check_overlaps(c, who, ncomp, {U}, {{phi, "phi must not overlap U, p or nrhs"}, {p, "p must not overlap U or nrhs"},
                                                    {nrhs, "nrhs must not overlap U"}}, bcv)) return rc;
  PaRange range_("pyapes projection update");
  PA_HIP(c, hipSetDevice(c->device));
  return c->dtype == PA_F64 ? correct_t<double>(c, U, ncomp, phi, scale, U, p, nrhs, chi, bcv)
                            : correct_t<float>(c, U, ncomp, phi, scale, U, p, nrhs, chi, bcv);
}

}  // extern "C"
