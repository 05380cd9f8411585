// pa_project.hip -- the two streaming kernels of the pressure projection (DESIGN.md section 4 "Projection") and their entry
// points: pa_divergence, the collocated central divergence of a vector field in one pass, and pa_project_correct, the gradient
// correction of every component in one launch followed by the ordered BC fill per component.
//
// The arithmetic is a definition of this library (the reference has no counterpart).  Per active internal axis a, every
// operation rounded on its own in the grid dtype (no FMA), h_a = 0.5 / dx_a formed in double on the host and converted once:
//   divergence   d = U_a[+1]_a - U_a[-1]_a;  d = d * h_a;  s = s + d   (s starts at +0, axes ascending);   out = scale * s
//   correction   g = p[+1]_c - p[-1]_c;  g = g * h_c;  g = scale * g;  out_c = U_c - g
// on the interior set (pa_in_S); off it the divergence is +0 and the correction hands U_c on.  Neighbours wrap around like
// every stencil of the library (pa_nbrs), and are read from the BC-filled input: the caller filled it.
//
// One cell per lane, a grid-stride loop under PA_MAX_GRID: both kernels move (d + 1) / (2 d + 1) arrays and compute next to
// nothing, so there is nothing to tile.  The streams touched once -- the divergence's `out`, the old U of the correction -- go
// past the caches as non-temporal accesses; the neighbour reads of U / p are plain loads, which the caches serve.
#include "pa_host.h"

#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>

// one pointer per INTERNAL axis (a d-dimensional mesh occupies the last d), the ghost planes being the field's own wrap-around
// planes; h[a] = (T)(0.5 / dx_a)
template <typename T>
struct ProjVec {
  Vec<T> v[3];
  T h[3];
};

template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_divergence(DevGeom G, ProjVec<T> U, T scale, T* __restrict__ out) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < G.ncell;
       idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t i, j, k;
    pa_decode(G, idx, i, j, k);
    T v = (T)0;
    if (pa_in_S(G, i, j, k)) {
      T s = (T)0;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        if (!G.act[a]) continue;
        FieldAcc<T> acc{U.v[a]};
        T xp, xm;
        pa_nbrs<T>(G, acc, a, i, j, k, xp, xm);
        T d = xp - xm;
        d = d * U.h[a];
        s = s + d;
      }
      v = scale * s;
    }
    __builtin_nontemporal_store(v, out + idx);
  }
}

// U.v[a].p: component of internal axis a, read at the cell only; o[a]: where it goes (o[a] == U.v[a].p: in place -- a cell's
// value is read and written by the same lane, and no lane reads another cell of U)
template <typename T>
struct ProjOut { T* o[3]; };

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
      T v = __builtin_nontemporal_load(U.v[a].p + idx);
      if (in) {
        T xp, xm;
        pa_nbrs<T>(G, acc, a, i, j, k, xp, xm);
        T g = xp - xm;
        g = g * U.h[a];
        g = scale * g;
        v = v - g;
      }
      O.o[a][idx] = v;
    }
  }
}

// PYAPES_HIP_DEBUG: one line per launch, `budget` of them per print site
static bool proj_dbg(int* left, int budget) {
  if (*left < 0) *left = getenv("PYAPES_HIP_DEBUG") ? budget : 0;
  if (*left <= 0) return false;
  --*left;
  return true;
}

template <typename T>
static ProjVec<T> proj_vec(const pa_ctx* c, const void* U) {
  ProjVec<T> P;
  const int sh = 3 - c->ndim;
  for (int a = 0; a < 3; ++a) {
    const T* comp = (const T*)U + (int64_t)(a >= sh ? a - sh : 0) * c->G.ncell;   // (an inactive axis: never read)
    P.v[a] = pa_vec_self<T>(c, comp);
    P.h[a] = (T)(0.5 / c->dx[a]);
  }
  return P;
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

// the kernel, then -- bcv non-null -- the ordered BC fill of every component with that component's face values in the bound
// list (types, order and dxf stay: pa_momentum_march's mechanism); the list is restored on every way out
template <typename T>
static int correct_t(pa_ctx* c, const void* U, int ncomp, const void* p, double scale, void* out, const pa_bc_values* bcv) {
  static int dbg = -1;
  if (proj_dbg(&dbg, 64))
    fprintf(stderr, "[pyapes_hip] k_project_correct%s: generic kernel, %lld cells\n", out == U ? " (in place)" : "", (long long)c->G.ncell);
  const int sh = 3 - c->ndim;
  const int64_t nc = c->G.ncell;
  ProjOut<T> O;
  for (int a = 0; a < 3; ++a) O.o[a] = (T*)out + (int64_t)(a >= sh ? a - sh : 0) * nc;
  hipLaunchKernelGGL(k_project_correct<T>, dim3(pa_grid_blocks(nc)), dim3(PA_BLOCK), 0, c->stream, c->G, proj_vec<T>(c, U),
                     pa_vec_self<T>(c, (const T*)p), (T)scale, O);
  PA_HIP(c, hipGetLastError());
  if (!bcv) return PA_OK;
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

// [p, p + pbytes) against the buffers of a call, each `bbytes` long (null entries: not part of the call)
static bool overlaps(const void* p, size_t pbytes, std::initializer_list<const void*> bufs, size_t bbytes) {
  for (const void* b : bufs)
    if (p && b && (const char*)p < (const char*)b + bbytes && (const char*)b < (const char*)p + pbytes) return true;
  return false;
}

// the refusals both entry points share, made before anything is enqueued
static int check_projection_call(pa_ctx* c, const char* who, int ncomp) {
  if (!c || !c->grid_set) return PA_E_STATE;
  if (c->slab || (c->G.n0 != c->G.g0 && c->ndim == 3)) { pa_set_err(c, "%s: single GPU only (no slabs)", who); return PA_E_STATE; }
  if (c->solve != PA_SOLVE_NONE) { pa_set_err(c, "%s during a stepwise solve (pa_cg_begin ... pa_cg_end); end or abort it first", who); return PA_E_STATE; }
  if (c->coord != PA_COORD_XYZ) { pa_set_err(c, "%s: for xyz meshes (no axisymmetric rows)", who); return PA_E_ARG; }
  if (c->ndim < 2 || ncomp != c->ndim) {
    pa_set_err(c, "%s: one component per mesh axis on a 2-D or 3-D mesh (%d components, %d axes)", who, ncomp, c->ndim);
    return PA_E_ARG;
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
  const size_t cbytes = (size_t)c->G.ncell * c->esize, vbytes = cbytes * (size_t)ncomp;
  if (overlaps(p, cbytes, {U, out}, vbytes)) { pa_set_err(c, "%s: p must not overlap U or out", who); return PA_E_ARG; }
  if (out != U && overlaps(out, vbytes, {U}, vbytes)) { pa_set_err(c, "%s: out is U itself (in place) or a buffer of its own", who); return PA_E_ARG; }
  if (bcv) {
    const int64_t n[3] = {c->G.n0, c->G.n1, c->G.n2};
    for (int q = 0; q < ncomp; ++q)
      for (int f = 0; f < 2 * c->ndim; ++f) {
        const size_t fbytes = cbytes / (size_t)n[(f >> 1) + 3 - c->ndim];
        if (overlaps(bcv[q].vals[f], fbytes, {U, out}, vbytes) || overlaps(bcv[q].vals[f], fbytes, {p}, cbytes)) {
          pa_set_err(c, "%s: a BC face array must not overlap a buffer of the call", who);
          return PA_E_ARG;
        }
      }
  }
  PaRange range_("pyapes projection correction");
  PA_HIP(c, hipSetDevice(c->device));
  return c->dtype == PA_F64 ? correct_t<double>(c, U, ncomp, p, scale, out, bcv) : correct_t<float>(c, U, ncomp, p, scale, out, bcv);
}

}  // extern "C"
