// pa_solver.hip -- what the CG / Jacobi / BiCGSTAB drivers (pa_cg.hip, pa_jacobi.hip, pa_bicgstab.hip) share: the
// first-residual kernels, the guarded copy and the plane packing, the device-resident scalars and their polls, the
// one-shot drivers' resident attempt and timed tail, the solve-state guard, and the method-neutral entry points.
#include "pa_solver.h"

// ---- the first residual: r = (b - A x) on S (0 elsewhere), d = r, partial sum r.r (linalg.py:98-107) ---------------
// One loop, grid and partial sum; two choices.
//   TERMS  A x from the generic term evaluation on xv; else from the array `ax`, where a tiled kernel left it (zero
//          outside S; `ax` may be r itself) -- r, d and the sum r.r come out bit-identical either way.
//   PITCH  r and d leave with a row pitch of ps1 cells, pad cells zero (the PITCH layout of the tiled phases,
//          pa_cg3d_kernel.h: odd row lengths); else contiguous, d optional, with the send planes of a slab.
template <typename T, bool TERMS, bool PITCH>
__global__ void __launch_bounds__(PA_BLOCK) k_cg_init(DevGeom G, DevEq<T> E, Vec<T> xv, const T* rhs,
                                                       const T* ax, T* r,   // (rhs and ax may be r)
                                                       T* __restrict__ d, T* __restrict__ send_lo,
                                                       T* __restrict__ send_hi, int64_t ps1, double* __restrict__ partials) {
  FieldAcc<T> acc{xv};
  double s[1] = {0.0};
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t idx = t0; idx < G.ncell; idx += stride) {
    int64_t i, j, k;
    pa_decode(G, idx, i, j, k);
    T rv = (T)0;
    if (pa_in_S(G, i, j, k)) {
      T axv;
      if constexpr (TERMS) axv = pa_apply_terms<T>(G, E, acc, i, j, k, xv.p[idx]);
      else axv = ax[idx];
      rv = rhs[idx] - axv;
      T p = rv * rv;
      s[0] += (double)p;
    }
    if constexpr (PITCH) {
      const int64_t o = (i * G.n1 + j) * ps1 + k;
      r[o] = rv;
      d[o] = rv;
    } else {
      r[idx] = rv;
      if (d) d[idx] = rv;
      if (send_lo && i == 0) send_lo[j * G.s1 + k] = rv;
      if (send_hi && i == G.n0 - 1) send_hi[j * G.s1 + k] = rv;
    }
  }
  if constexpr (PITCH) {
    const int64_t rows = G.n0 * G.n1, pw = ps1 - G.n2;
    for (int64_t q = t0; q < rows * pw; q += stride) {
      const int64_t o = (q / pw) * ps1 + G.n2 + q % pw;
      r[o] = (T)0;
      d[o] = (T)0;
    }
  }
  pa_block_reduce_store<1>(s, partials);
}

template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_cg_post_init(SolverScalars* sc, const double* partials, int nblk,
                                                            double* sums, int stage) {
  __shared__ double sm[PA_BLOCK / 64];
  if (stage != 1) {
    double v = pa_reduce_partials(partials, nblk, 1, 0, sm);
    if (threadIdx.x == 0) sums[1] = v;
  }
  if (stage != 0 && threadIdx.x == 0) sc->rr = (double)(T)sums[1];
}

// slab, periodic axis 0: copies of the x planes the other end rank's BC fill needs, placed next to
// the residual planes in the packed send buffers (one message per neighbour and iteration)
template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_pack_planes(const SolverScalars* __restrict__ sc, int64_t n,
                                                           const T* __restrict__ s0, T* __restrict__ d0,
                                                           const T* __restrict__ s1, T* __restrict__ d1,
                                                           const T* __restrict__ s2, T* __restrict__ d2) {
  if (sc->done) return;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
    if (d0) d0[q] = s0[q];
    if (d1) d1[q] = s1[q];
    if (d2) d2[q] = s2[q];
  }
}

// x_old of the iteration that is about to update x (skipped, like the update, once the solve is over)
template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_copy_guarded(const SolverScalars* __restrict__ sc, const T* __restrict__ a,
                                                            T* __restrict__ b, int64_t n) {
  if (sc->done) return;
  typedef T V __attribute__((ext_vector_type(16 / sizeof(T))));
  constexpr int VEC = 16 / sizeof(T);
  const bool vec = (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
  const int64_t nv = vec ? n / VEC : 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x)
    reinterpret_cast<V*>(b)[i] = reinterpret_cast<const V*>(a)[i];
  for (int64_t i = nv * VEC + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    b[i] = a[i];
}

// ---- host side ----------------------------------------------------------------------------------
int init_scalars(pa_ctx* c, double tol, int64_t max_it) {
  SolverScalars h;
  memset(&h, 0, sizeof(h));
  h.tolerance = tol;
  h.max_it = max_it;
  h.tol = 1.0;
  h.rho = 1.0; h.alpha = 1.0; h.omega = 1.0;
  h.done = !(1.0 > tol);  // `while tol > tolerance` with tol = 1.0 (linalg.py:90,109)
  *c->h_sc = h;
  PA_HIP(c, hipMemcpyAsync(c->sc, c->h_sc, sizeof(h), hipMemcpyHostToDevice, c->stream));
  PA_HIP(c, hipStreamSynchronize(c->stream));
  return PA_OK;
}

int read_scalars(pa_ctx* c) {
  PA_HIP(c, hipMemcpyAsync(c->h_sc, c->sc, sizeof(SolverScalars), hipMemcpyDeviceToHost, c->stream));
  PA_HIP(c, hipStreamSynchronize(c->stream));
  return PA_OK;
}

int poll_submit(pa_ctx* c, PollPipe& P, bool* done) {
  *done = false;
  PA_HIP(c, hipMemcpyAsync(c->h_poll[P.slot], c->sc, sizeof(SolverScalars), hipMemcpyDeviceToHost, c->stream));
  PA_HIP(c, hipEventRecord(c->ev_poll[P.slot], c->stream));
  if (P.pending >= 0) {
    PA_HIP(c, hipEventSynchronize(c->ev_poll[P.pending]));
    *done = c->h_poll[P.pending]->done != 0;
  }
  P.pending = P.slot;
  P.slot ^= 1;
  return PA_OK;
}
int poll_drain(pa_ctx* c, PollPipe& P, bool* done) {
  *done = false;
  if (P.pending < 0) return PA_OK;
  PA_HIP(c, hipEventSynchronize(c->ev_poll[P.pending]));
  *done = c->h_poll[P.pending]->done != 0;
  P.pending = -1;
  return PA_OK;
}

int poll_interval(const pa_ctx* c) {
  // keep >= ~300 us of queued GPU work between host polls of the done flag
  double est_us = (double)c->G.ncell * 80.0 / 4.0e6 + 30.0;
  int k = (int)ceil(300.0 / est_us);
  return std::max(1, std::min(k, 64));
}

static void fill_report(pa_ctx* c, pa_report* out, float ms) {
  const SolverScalars& h = *c->h_sc;
  out->itr = h.itr;
  out->tol = h.tol;
  out->converge = h.itr < h.max_it;
  out->status = h.err ? PA_E_NONFINITE : PA_OK;
  out->rr = h.rr;
  out->gpu_ms = ms;
}

template <typename T>
int try_resident(pa_ctx* c, int kind, T* x, const T* rhs, double tol, int64_t max_it, double omega, pa_report* out,
                 int* rc) {
  const hipError_t e0 = hipEventRecord(c->ev0, c->stream);
  if (e0 != hipSuccess) { *rc = pa_hip_fail(c, e0, "hipEventRecord(c->ev0, c->stream)"); return 1; }
  c->resident_used = pa_resident_launch<T>(c, kind, x, rhs, tol, max_it, omega);
  if (c->resident_used < 0) { *rc = c->resident_used; return 1; }
  if (c->resident_used == 0) return 0;
  int* h_fail = (int*)&c->h_poll[0]->rr;   // pinned scratch (the poll slots are idle here)
  *h_fail = 0;
  hipError_t e = hipMemcpyAsync(h_fail, (const char*)c->scr[SCR_RES] + 64, sizeof(int), hipMemcpyDeviceToHost, c->stream);
  if (e != hipSuccess) { *rc = pa_hip_fail(c, e, "resident fail flag"); return 1; }
  if ((*rc = read_scalars(c))) { c->solve = PA_SOLVE_NONE; return 1; }   // (synchronises the stream)
  if (*h_fail) { c->resident_used = 0; return 0; }   // it gave up: on as if the launch had not happened
  c->solve = PA_SOLVE_NONE;
  *rc = timed_report(c, out);
  return 1;
}

int timed_report(pa_ctx* c, pa_report* out) {
  PA_HIP(c, hipEventRecord(c->ev1, c->stream));
  PA_HIP(c, hipEventSynchronize(c->ev1));
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
  fill_report(c, out, ms);
  return c->h_sc->err ? PA_E_NONFINITE : PA_OK;
}

// r = (b - A x) on S (0 elsewhere), d = r, per-block partial sums of r.r: the tiled A x kernel plus one
// streaming pass where the tiled kernel applies, else the generic kernel
template <typename T>
int cg_residual_init(pa_ctx* c, const DevEq<T>& E, Vec<T> xv, const T* rhs, T* r, T* d, T* send_lo, T* send_hi,
                     double* part) {
  const int nblk = pa_grid_blocks(c->G.ncell);
  // slab: a NULL ghost plane marks a physical (non-periodic) end.  No result ever uses that plane (the
  // end plane is a boundary node, outside S), but the tiled kernel loads it speculatively: the field's
  // own end plane stands in, so the load stays inside valid memory.
  Vec<T> xt = xv;
  if (!xt.glo) xt.glo = xt.p;
  if (!xt.ghi) xt.ghi = xt.p + (c->G.n0 - 1) * c->G.s0;
  int fr = (rhs != r && (const T*)xv.p != r) ? pa_tile3d_aop<T>(c, E, xt, r, 1) : 0;
  if (fr < 0) return fr;
  if (fr > 0)   // (A x sits in r)
    hipLaunchKernelGGL((k_cg_init<T, false, false>), dim3(nblk), dim3(PA_BLOCK), 0, c->stream, c->G, E, xv, rhs, (const T*)r,
                       r, d, send_lo, send_hi, (int64_t)0, part);
  else
    hipLaunchKernelGGL((k_cg_init<T, true, false>), dim3(nblk), dim3(PA_BLOCK), 0, c->stream, c->G, E, xv, rhs,
                       (const T*)nullptr, r, d, send_lo, send_hi, (int64_t)0, part);
  return PA_OK;
}

template <typename T>
int cg_residual_init_pitch(pa_ctx* c, const DevEq<T>& E, Vec<T> xv, const T* rhs, T* ax, T* r, T* d, double* part) {
  const int nblk = pa_grid_blocks(c->G.ncell);
  const int fr = pa_tile3d_aop<T>(c, E, xv, ax, 1);
  if (fr < 0) return fr;
  if (fr > 0) {
    hipLaunchKernelGGL((k_cg_init<T, false, true>), dim3(nblk), dim3(PA_BLOCK), 0, c->stream, c->G, E, xv, rhs, (const T*)ax,
                       r, d, (T*)nullptr, (T*)nullptr, c->cg_ps1, part);
  } else if (c->coord == PA_COORD_RZ) {   // no tiled A x with r rows: the generic term evaluation, once per solve
    hipLaunchKernelGGL((k_cg_init<T, true, true>), dim3(nblk), dim3(PA_BLOCK), 0, c->stream, c->G, E, xv, rhs,
                       (const T*)nullptr, r, d, (T*)nullptr, (T*)nullptr, c->cg_ps1, part);
  } else {   // the tiled A x declined: contiguous layout (the buffers are merely larger)
    c->cg_pitch = 0, c->cg_ps1 = 0;
  }
  return PA_OK;
}

// Row pitch (cells) of the ctx-owned solver arrays when the PITCH layout applies to a solve on x, else 0.
// Row lengths that are not a multiple of the 16-byte vector -- the normal case of a node-based mesh (11, 101,
// 2^k + 1 nodes: _mesh.py:67-93) -- on one GPU: the arrays the ctx owns get a row pitch rounded up (PITCH layout of
// k_cg3d), so the solver phases keep their 16-byte lane accesses on everything but the caller's x.  Needs a
// non-periodic contiguous axis (a pad cell must never be a neighbour that is used) and a plain Laplacian; everything
// else stays on the one-cell-per-lane (NARROW) kernels.
template <typename T>
int64_t solver_pitch(const pa_ctx* c, const T* x) {
  const DevGeom& G = c->G;
  constexpr int VECW = 16 / (int)sizeof(T);
  const bool shape = (c->ndim == 3 && G.n0 >= 3 && G.n1 >= 3) || (c->ndim == 2 && G.n1 >= 3);
  // (axisymmetric meshes: their one tiled kernel is the 2-D marching k_cg2d<..., RZ>, pa_cg2d_kernel.h)
  const bool coord_ok = c->coord == PA_COORD_XYZ ||
                        (c->coord == PA_COORD_RZ && c->ndim == 2 && c->rz_tab && G.n1 >= 8 && c->cg2d_mincells >= 0 &&
                         G.n1 * G.n2 >= std::min<int64_t>(c->cg2d_mincells, 150000));
  if (!(c->pitch && c->fastpath && !c->slab && coord_ok && shape && G.n2 % VECW != 0 && G.n2 >= 2 * VECW &&
        c->nterms == 1 && c->terms[0].kind == PA_OP_LAPLACIAN && !c->terms[0].coeff_field &&
        G.bct[4] != PA_BC_PERIODIC && G.bct[5] != PA_BC_PERIODIC && ((uintptr_t)x & (sizeof(T) - 1)) == 0 &&
        ((G.n1 + 3) / 4) * ((G.n2 + 64 * VECW - 1) / (64 * VECW)) <= PA_MAX_PARTIALS))
    return 0;
  // pitch: a multiple of 128 bytes, not merely of the vector -- measured at 257^3 fp64 with 16-byte granularity
  // (258 cells): phase A 108 us against 79 at 256^3 on the same tiling, although every access was a vector:
  // rows that start inside a cache line make every tile edge a line shared by two workgroups, and their
  // streaming stores partial-line writes
  const int64_t padw = 128 / (int64_t)sizeof(T);
  return (G.n2 + padw - 1) / padw * padw;
}

// profiling build of the launch path: HIP events on the ctx stream bracket exactly one
// dominant kernel; the host waits for each, so use it in a dedicated measurement loop only
void pa_profile_stop(pa_ctx* c, int which) {
  hipEvent_t e0 = c->pev[2 * which], e1 = c->pev[2 * which + 1];
  (void)hipEventRecord(e1, c->stream);
  (void)hipEventSynchronize(e1);
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) {
    c->prof_ms[which] += ms;
    c->prof_n[which] += 1;
  }
}

template <typename T>
Vec<T> slab_vec(const pa_ctx* c, const T* p, const void* glo, const void* ghi) {
  Vec<T> v;
  v.p = p;
  v.glo = glo ? (const T*)glo : p;
  v.ghi = ghi ? (const T*)ghi : p + (c->G.n0 - 1) * c->G.s0;
  return v;
}

template <typename T>
void launch_post_init(pa_ctx* c, const double* part, int nblk, int stage) {
  hipLaunchKernelGGL(k_cg_post_init<T>, dim3(1), dim3(PA_BLOCK), 0, c->stream, c->sc, part, nblk, pa_sums(c), stage);
}

template <typename T>
void copy_x_old(pa_ctx* c, const T* x) {
  if (c->x_old_out)
    hipLaunchKernelGGL(k_copy_guarded<T>, dim3(pa_grid_blocks(c->G.ncell)), dim3(PA_BLOCK), 0, c->stream, c->sc, x,
                       (T*)c->x_old_out, c->G.ncell);
}

template <typename T>
void pack_x_planes(pa_ctx* c, const T* x) {
  const DevGeom& G = c->G;
  if (c->x_pack_lo1 || c->x_pack_hi0 || c->x_pack_hi1)
    hipLaunchKernelGGL(k_pack_planes<T>, dim3(pa_grid_blocks(G.s0)), dim3(PA_BLOCK), 0, c->stream, c->sc, G.s0,
                       x + 1 * G.s0, (T*)c->x_pack_lo1, x + (G.n0 - 1) * G.s0, (T*)c->x_pack_hi0,
                       x + (G.n0 - 2) * G.s0, (T*)c->x_pack_hi1);
}

template <typename T>
void pack_end_planes(pa_ctx* c, const T* a, void* lo, void* hi) {
  const DevGeom& G = c->G;
  if (lo || hi)
    hipLaunchKernelGGL(k_pack_planes<T>, dim3(pa_grid_blocks(G.s0)), dim3(PA_BLOCK), 0, c->stream, c->sc, G.s0,
                       a, (T*)lo, a + (G.n0 - 1) * G.s0, (T*)hi, (const T*)nullptr, (T*)nullptr);
}

#define PA_SOLVER_INST(T)                                                                                         \
  template int try_resident<T>(pa_ctx*, int, T*, const T*, double, int64_t, double, pa_report*, int*);           \
  template int cg_residual_init<T>(pa_ctx*, const DevEq<T>&, Vec<T>, const T*, T*, T*, T*, T*, double*);         \
  template int cg_residual_init_pitch<T>(pa_ctx*, const DevEq<T>&, Vec<T>, const T*, T*, T*, T*, double*);       \
  template int64_t solver_pitch<T>(const pa_ctx*, const T*);                                                     \
  template Vec<T> slab_vec<T>(const pa_ctx*, const T*, const void*, const void*);                                \
  template void launch_post_init<T>(pa_ctx*, const double*, int, int);                                           \
  template void copy_x_old<T>(pa_ctx*, const T*);                                                                \
  template void pack_x_planes<T>(pa_ctx*, const T*);                                                             \
  template void pack_end_planes<T>(pa_ctx*, const T*, void*, void*);
PA_SOLVER_INST(float)
PA_SOLVER_INST(double)
#undef PA_SOLVER_INST

static const char* const solve_name[] = {"", "CG", "BiCGSTAB", "Jacobi"};
static const char* const solve_begin[] = {"", "pa_cg_begin", "pa_bicg_begin", "pa_jacobi_begin"};

int pa_require_solve(pa_ctx* c, PaSolve kind, const char* what) {
  if (!c) return PA_E_STATE;
  if (c->solve != kind) {
    if (c->solve == PA_SOLVE_NONE) pa_set_err(c, "%s without %s", what, solve_begin[kind]);
    else pa_set_err(c, "%s during a stepwise %s solve", what, solve_name[c->solve]);
    return PA_E_STATE;
  }
  PA_HIP(c, hipSetDevice(c->device));
  return PA_OK;
}

extern "C" {

int pa_solver_keep_old(pa_ctx* c, void* x_old) {
  if (!c) return PA_E_ARG;
  if (x_old && c->solve != PA_SOLVE_NONE) { pa_set_err(c, "pa_solver_keep_old during a solve"); return PA_E_STATE; }
  c->x_old_out = x_old;
  return PA_OK;
}

int pa_profile_set(pa_ctx* c, int on) {
  if (!c) return PA_E_ARG;
  if (on && !c->pev[0])
    for (int q = 0; q < 4; ++q) PA_HIP(c, hipEventCreate(&c->pev[q]));
  c->profile = on ? 1 : 0;
  c->prof_ms[0] = c->prof_ms[1] = 0.0;
  c->prof_n[0] = c->prof_n[1] = 0;
  return PA_OK;
}

int pa_profile_read(pa_ctx* c, double* ms_a, int64_t* n_a, double* ms_b, int64_t* n_b) {
  if (!c) return PA_E_ARG;
  if (ms_a) *ms_a = c->prof_ms[0];
  if (n_a) *n_a = c->prof_n[0];
  if (ms_b) *ms_b = c->prof_ms[1];
  if (n_b) *n_b = c->prof_n[1];
  return PA_OK;
}

int pa_report_read(pa_ctx* c, pa_report* out) {
  if (!c || !out) return PA_E_ARG;
  int rc = read_scalars(c);
  if (rc) return rc;
  fill_report(c, out, 0.f);
  return PA_OK;
}

int pa_scalars_read(pa_ctx* c, double* out) {
  if (!c || !out) return PA_E_ARG;
  if (c->solve != PA_SOLVE_NONE) {   // a stepwise solve: fetch the live state; after pa_cg / pa_bicgstab / pa_jacobi the mirror is current
    int rc = read_scalars(c);
    if (rc) return rc;
  }
  const SolverScalars& h = *c->h_sc;
  const double v[PA_NSCALAR] = {h.alpha, h.beta, h.rr, h.rr_old, h.dAd, h.tol, h.rho, h.omega, h.rho_next, h.r0v,
                                h.ts, h.tt, h.r0t, (double)h.itr, 0.0, 0.0};
  for (int q = 0; q < PA_NSCALAR; ++q) out[q] = v[q];
  return PA_OK;
}

int pa_cg_abort(pa_ctx* c) {   // drop the live stepwise solve, whichever method, without reading it back
  if (!c) return PA_E_ARG;
  c->solve = PA_SOLVE_NONE;
  c->in_iterate = c->slab_fold_live = 0;
  c->fold_a_n = c->fold_b_n = c->fold_b_nsh = 0;
  c->fold_b_shell = nullptr;
  pa_place_end(c, 0);   // (no hipFree here: it would wait for a stream that may never drain)
  return PA_OK;
}

}  // extern "C"
