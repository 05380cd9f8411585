// pa_jacobi.hip -- damped Jacobi [new, SURVEY a15]: the generic sweep, the one-shot driver (pa_jacobi) and the
// stepwise form on a slab.
#include "pa_solver.h"

// ---- Jacobi sweep [new, SURVEY a15] -----------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_jacobi(DevGeom G, DevEq<T> E, const SolverScalars* __restrict__ sc,
                                                      Vec<T> xv, const T* __restrict__ rhs,
                                                      T* __restrict__ xnew, T omega,
                                                      double* __restrict__ partials) {
  if (sc->done) return;
  FieldAcc<T> acc{xv};
  double s[2] = {0.0, 0.0};
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < G.ncell;
       idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t i, j, k;
    pa_decode(G, idx, i, j, k);
    T xo = xv.p[idx];
    T xn = xo;
    if (pa_in_S(G, i, j, k)) {
      int64_t g[3], N[3];
      pa_gidx(G, i, j, k, g, N);
      T diag = (T)0;
      for (int q = 0; q < E.nterms; ++q) {
        const DevTerm<T>& t = E.t[q];
        T dg = (T)0;
        for (int a = 0; a < 3; ++a) {
          if (!G.act[a]) continue;
          int rc = pa_row_case(G, a, g[a], N[a], G.treat);
          T cB = (E.rz && a == PA_RZ_AXIS) ? E.rz[2 * E.rz_n + g[a]] : E.lap.c23[a];
          T cC = rc == 0 ? E.lap.m2inv[a] : -cB;
          dg = dg + cC;
        }
        if (t.has_coeff) dg = dg * (t.coeff_f ? t.coeff_f[idx] : t.coeff);
        dg = dg * t.sign;
        diag = diag + dg;
      }
      T ax = pa_apply_terms<T>(G, E, acc, i, j, k, xo);
      T res = rhs[idx] - ax;
      res = res / diag;
      T w = omega * res;
      xn = xo + w;
      if (!pa_on_shell(G, i, j, k)) {
        T df = xn - xo;
        T p2 = df * df;
        s[1] += (double)p2;
      }
    }
    xnew[idx] = xn;
  }
  pa_block_reduce_store<2>(s, partials);
}

template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_jacobi_post(SolverScalars* sc, const double* partials, int nblk,
                                                           const double* partials_shell, int nblk_shell,
                                                           double* sums) {
  __shared__ double sm[PA_BLOCK / 64];
  if (sc->done) return;
  double dx2 = pa_reduce_partials(partials, nblk, 2, 1, sm);
  double sh = nblk_shell > 0 ? pa_reduce_partials(partials_shell, nblk_shell, 1, 0, sm) : 0.0;
  if (threadIdx.x == 0) {
    sums[2] = dx2 + sh;
    pa_logic_jacobi<T>(sc, sums[2]);
  }
}

template <typename T>
__global__ void k_copy(const T* __restrict__ a, T* __restrict__ b, int64_t n) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n;
       idx += (int64_t)gridDim.x * blockDim.x)
    b[idx] = a[idx];
}

template <typename T>
static int jacobi_run_t(pa_ctx* c, T* x, const T* rhs, double tol, int64_t max_it, double omega, pa_report* out) {
  const DevGeom& G = c->G;
  for (int q = 0; q < c->nterms; ++q)
    if (c->terms[q].kind != PA_OP_LAPLACIAN) { pa_set_err(c, "pa_jacobi: laplacian terms only"); return PA_E_ARG; }
  if (c->slab) { pa_set_err(c, "pa_jacobi is single-GPU only"); return PA_E_ARG; }
  int rc;
  c->jac_dir = 0;   // every solve starts with a forward sweep, whatever ran on this context before (the stop-test sum is ordered by it)
  if (try_resident<T>(c, 1, x, rhs, tol, max_it, omega, out, &rc)) return rc;
  const size_t fb = (size_t)G.ncell * sizeof(T);
  const int nblk = pa_grid_blocks(G.ncell);
  if ((rc = pa_scratch(c, &c->scr[SCR_D0], &c->cap[SCR_D0], fb))) return rc;
  if ((rc = pa_scratch(c, &c->scr[SCR_PART], &c->cap[SCR_PART], (size_t)PA_MAX_PARTIALS * 4 * sizeof(double)))) return rc;
  if ((rc = pa_scratch(c, &c->scr[SCR_PART2], &c->cap[SCR_PART2], (size_t)3 * PA_MAX_GRID * sizeof(double)))) return rc;
  if ((rc = pa_scratch(c, &c->scr[SCR_SHELL], &c->cap[SCR_SHELL], 2 * (size_t)pa_shell_elems(c) * sizeof(T)))) return rc;
  if ((rc = init_scalars(c, tol, max_it))) return rc;
  DevEq<T> E;
  pa_build_eq<T>(c, c->nterms, c->terms, E);
  double* part = (double*)c->scr[SCR_PART];
  double* part2 = (double*)c->scr[SCR_PART2];
  // BC fill by the cheapest launch sequence, as in CG: closed form / one launch per axis / one per face
  pa_bc_plan(c);
  c->fold_a_n = c->fold_b_n = c->fold_b_nsh = 0;
  if ((rc = pa_bc_fill_start<T>(c, x, false))) return rc;
  T* buf[2] = {x, (T*)c->scr[SCR_D0]};
  int cur = 0;
  const int poll = poll_interval(c);
  PA_HIP(c, hipEventRecord(c->ev0, c->stream));
  int64_t enq = 0;
  // the stop test of sweep q is left to the prologue of sweep q+1 (pa_cg3d_kernel.h) when both are
  // tiled; this runs it as the single-block kernel it replaces (before a poll, before a generic sweep)
  auto flush = [&]() {
    if (c->fold_b_n > 0)
      hipLaunchKernelGGL(k_jacobi_post<T>, dim3(1), dim3(PA_BLOCK), 0, c->stream, c->sc, c->fold_b_part, c->fold_b_n,
                         (const double*)part2, c->fold_b_nsh, pa_sums(c));
    c->fold_b_n = c->fold_b_nsh = 0;
  };
  PollPipe P;
  bool done = false;
  int64_t batch = 2;
  while (!done) {
    // the device stops by itself after max_it + 1 sweeps; sweeps are enqueued in pairs
    int64_t nb = std::min<int64_t>(batch, max_it + 2 - enq);
    if (nb <= 0) {
      if ((rc = poll_drain(c, P, &done))) return rc;
      if (done) break;
      nb = 2;
    }
    // two sweeps per round so that the iterate is back in the caller's buffer at every poll
    for (int64_t half = 0; half < ((nb + 1) & ~(int64_t)1); ++half) {
      Vec<T> xv = pa_vec_self<T>(c, buf[cur]);
      // partial rows alternate between the halves of SCR_PART: the next sweep reads these while it writes its own
      double* part_q = part + (cur ? 2 * (size_t)PA_MAX_PARTIALS : 0);
      if (c->profile) (void)hipEventRecord(c->pev[0], c->stream);   // slot 0: the sweep kernel
      int used = pa_tile3d_jacobi<T>(c, E, xv, rhs, buf[cur ^ 1], omega, part_q);
      if (used < 0) return used;
      const bool tiled = used > 0;
      if (!tiled) {
        flush();
        hipLaunchKernelGGL(k_jacobi<T>, dim3(nblk), dim3(PA_BLOCK), 0, c->stream, G, E, c->sc, xv, rhs, buf[cur ^ 1],
                           (T)omega, part_q);
        used = nblk;
      }
      if (c->profile) pa_profile_stop(c, 0);
      int nsh;
      // NOTE: when done is set the sweep kernels return early, so buf[cur^1] is stale: the copy-back
      // below is guarded by the iteration parity recorded on the device (itr).
      if ((rc = pa_bc_fill_step<T>(c, buf[cur ^ 1], part2, &nsh))) return rc;
      if (c->fold && tiled && used <= PA_MAX_GRID && nsh <= 3 * PA_MAX_GRID) {
        c->fold_b_n = used;
        c->fold_b_nsh = nsh;
        c->fold_b_part = part_q;
      } else {
        hipLaunchKernelGGL(k_jacobi_post<T>, dim3(1), dim3(PA_BLOCK), 0, c->stream, c->sc, part_q, used, part2, nsh,
                           pa_sums(c));
      }
      cur ^= 1;
      ++enq;
    }
    flush();
    if ((rc = poll_submit(c, P, &done))) return rc;
    batch = std::min<int64_t>(2 * poll, std::max<int64_t>(2, enq));
  }
  if ((rc = read_scalars(c))) return rc;
  // the final iterate lives in buf[itr & 1], the one before it (Field.VARo) in the other buffer
  if (c->x_old_out && c->h_sc->itr >= 1)
    hipLaunchKernelGGL(k_copy<T>, dim3(nblk), dim3(PA_BLOCK), 0, c->stream, (const T*)buf[(c->h_sc->itr & 1) ^ 1],
                       (T*)c->x_old_out, G.ncell);
  if (c->h_sc->itr & 1) {
    hipLaunchKernelGGL(k_copy<T>, dim3(nblk), dim3(PA_BLOCK), 0, c->stream, (const T*)buf[1], x, G.ncell);
  }
  return timed_report(c, out);
}

extern "C" int pa_jacobi(pa_ctx* c, void* x, const void* rhs, double tol, int64_t max_it, double omega, pa_report* out) {
  if (!c || !c->grid_set || !c->eq_set) { if (c) pa_set_err(c, "pa_jacobi: grid/equation not set"); return PA_E_STATE; }
  if (int rc0 = pa_check_eq_applicable(c)) return rc0;
  if (!out) return PA_E_ARG;
  PA_HIP(c, hipSetDevice(c->device));
  return c->dtype == PA_F64 ? jacobi_run_t<double>(c, (double*)x, (const double*)rhs, tol, max_it, omega, out)
                            : jacobi_run_t<float>(c, (float*)x, (const float*)rhs, tol, max_it, omega, out);
}

// ============================================================================
//  stepwise Jacobi on a slab (SURVEY a15 + 8e): x <- B(x + omega (b - A x) / diag(A)), the CG's stop test
// ============================================================================
// Per sweep: the sweep kernel on the local planes (ghost planes of x through Vec<T>: pa_slab_set's x_ghost_lo / hi) ->
// [exchange of the periodic far planes of the NEW iterate] -> BC fill + shell term, local sum |dx|^2 -> sums[2]
// -> [all-reduce 1] -> stop test (device side) -> [exchange of the new iterate's first / last plane -> x_ghost].
// The iterate ping-pongs between the caller's x and a scratch field; the planes the neighbours need leave through the
// packed send buffers of pa_slab_set (r_send_lo / hi: first / last owned plane; x_pack_*: the periodic far planes).
template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_jacobi_rows_to_sum(const SolverScalars* __restrict__ sc, const double* __restrict__ partials,
                                                                  int nblk, const double* __restrict__ partials_shell, int nblk_shell,
                                                                  double* __restrict__ sums) {
  __shared__ double sm[PA_BLOCK / 64];
  if (sc->done) return;
  const double dx2 = pa_reduce_partials(partials, nblk, 2, 1, sm);
  const double sh = nblk_shell > 0 ? pa_reduce_partials(partials_shell, nblk_shell, 1, 0, sm) : 0.0;
  if (threadIdx.x == 0) sums[PA_SUM_DX2] = dx2 + sh;
}

template <typename T>
__global__ void k_jacobi_logic(SolverScalars* sc, const double* __restrict__ sums) {
  if (threadIdx.x != 0 || blockIdx.x != 0 || sc->done) return;
  pa_logic_jacobi<T>(sc, sums[PA_SUM_DX2]);
}

namespace {

template <typename T>
int jacobi_slab_begin_t(pa_ctx* c, T* x, const T* rhs, double tol, int64_t max_it, double omega) {
  const DevGeom& G = c->G;
  for (int q = 0; q < c->nterms; ++q)
    if (c->terms[q].kind != PA_OP_LAPLACIAN) { pa_set_err(c, "pa_jacobi_begin: laplacian terms only"); return PA_E_ARG; }
  const size_t fb = (size_t)G.ncell * sizeof(T);
  int rc;
  if ((rc = pa_scratch(c, &c->scr[SCR_D0], &c->cap[SCR_D0], fb))) return rc;
  if ((rc = pa_scratch(c, &c->scr[SCR_PART], &c->cap[SCR_PART], (size_t)PA_MAX_PARTIALS * 4 * sizeof(double)))) return rc;
  if ((rc = pa_scratch(c, &c->scr[SCR_PART2], &c->cap[SCR_PART2], (size_t)3 * PA_MAX_GRID * sizeof(double)))) return rc;
  if ((rc = pa_scratch(c, &c->scr[SCR_SHELL], &c->cap[SCR_SHELL], 2 * (size_t)pa_shell_elems(c) * sizeof(T)))) return rc;
  if ((rc = init_scalars(c, tol, max_it))) return rc;
  pa_bc_plan(c);
  c->fold_a_n = c->fold_b_n = c->fold_b_nsh = 0;
  c->cg_pitch = 0;
  c->cg_ps1 = 0;
  c->jac_dir = 0;   // the first sweep marches forwards: an earlier solve may have ended on an odd count of sweep launches
  // the driver has filled the BCs (it needs the far planes for that) and exchanged the ghost planes of x: only the
  // shell of the start is recorded here (x_old of the first stop test)
  if ((rc = pa_bc_fill_start<T>(c, x, true))) return rc;
  c->cg_x = x;
  c->jac_rhs = rhs;
  c->jac_omega = omega;
  c->cur = 0;            // the iterate lives in x (0) or in the scratch field (1)
  c->solve = PA_SOLVE_JACOBI;
  PA_HIP(c, hipGetLastError());
  return PA_OK;
}

template <typename T>
int jacobi_slab_sweep_t(pa_ctx* c) {
  const DevGeom& G = c->G;
  const int nblk = pa_grid_blocks(G.ncell);
  DevEq<T> E;
  pa_build_eq<T>(c, c->nterms, c->terms, E);
  T* buf[2] = {(T*)c->cg_x, (T*)c->scr[SCR_D0]};
  const int cur = c->cur;
  Vec<T> xv = slab_vec<T>(c, buf[cur], c->x_glo, c->x_ghi);
  double* part = (double*)c->scr[SCR_PART];
  c->fold_b_n = 0;
  int used = pa_tile3d_jacobi<T>(c, E, xv, (const T*)c->jac_rhs, buf[cur ^ 1], c->jac_omega, part);
  if (used < 0) return used;
  if (used == 0) {
    hipLaunchKernelGGL(k_jacobi<T>, dim3(nblk), dim3(PA_BLOCK), 0, c->stream, G, E, c->sc, xv, (const T*)c->jac_rhs, buf[cur ^ 1],
                       (T)c->jac_omega, part);
    used = nblk;
  }
  c->b_blocks = used;
  // the planes of the NEW iterate the other end of a periodic ring needs for its BC fill
  pack_x_planes<T>(c, buf[cur ^ 1]);
  PA_HIP(c, hipGetLastError());
  return PA_OK;
}

template <typename T>
int jacobi_slab_bc_t(pa_ctx* c) {
  T* buf[2] = {(T*)c->cg_x, (T*)c->scr[SCR_D0]};
  T* xn = buf[c->cur ^ 1];
  double* part = (double*)c->scr[SCR_PART];
  double* part2 = (double*)c->scr[SCR_PART2];
  int nsh, rc;
  if ((rc = pa_bc_fill_step<T>(c, xn, part2, &nsh))) return rc;
  hipLaunchKernelGGL(k_jacobi_rows_to_sum<T>, dim3(1), dim3(PA_BLOCK), 0, c->stream, c->sc, (const double*)part, c->b_blocks,
                     (const double*)part2, nsh, pa_sums(c));
  // the first / last owned plane of the new iterate, BCs filled: the neighbours' ghost planes of the next sweep
  pack_end_planes<T>(c, xn, c->r_send_lo, c->r_send_hi);
  PA_HIP(c, hipGetLastError());
  return PA_OK;
}

}  // namespace

extern "C" {

int pa_jacobi_begin(pa_ctx* c, void* x, const void* rhs, double tol, int64_t max_it, double omega) {
  if (!c || !c->grid_set || !c->eq_set) { if (c) pa_set_err(c, "pa_jacobi_begin: grid/equation not set"); return PA_E_STATE; }
  if (int rc0 = pa_check_eq_applicable(c)) return rc0;
  if (!c->slab || !c->ext_sums) { pa_set_err(c, "pa_jacobi_begin is the stepwise form for slabs (pa_slab_set); one GPU: pa_jacobi"); return PA_E_STATE; }
  PA_HIP(c, hipSetDevice(c->device));
  return c->dtype == PA_F64 ? jacobi_slab_begin_t<double>(c, (double*)x, (const double*)rhs, tol, max_it, omega)
                            : jacobi_slab_begin_t<float>(c, (float*)x, (const float*)rhs, tol, max_it, omega);
}

int pa_jacobi_sweep(pa_ctx* c) {
  if (int rc = pa_require_solve(c, PA_SOLVE_JACOBI, "pa_jacobi_sweep")) return rc;
  return c->dtype == PA_F64 ? jacobi_slab_sweep_t<double>(c) : jacobi_slab_sweep_t<float>(c);
}

int pa_jacobi_bc(pa_ctx* c) {
  if (int rc = pa_require_solve(c, PA_SOLVE_JACOBI, "pa_jacobi_bc")) return rc;
  return c->dtype == PA_F64 ? jacobi_slab_bc_t<double>(c) : jacobi_slab_bc_t<float>(c);
}

int pa_jacobi_finish(pa_ctx* c) {   // after the all-reduce of sums[PA_SUM_DX2]
  if (int rc = pa_require_solve(c, PA_SOLVE_JACOBI, "pa_jacobi_finish")) return rc;
  if (c->dtype == PA_F64) hipLaunchKernelGGL(k_jacobi_logic<double>, dim3(1), dim3(1), 0, c->stream, c->sc, (const double*)pa_sums(c));
  else hipLaunchKernelGGL(k_jacobi_logic<float>, dim3(1), dim3(1), 0, c->stream, c->sc, (const double*)pa_sums(c));
  c->cur ^= 1;
  PA_HIP(c, hipGetLastError());
  return PA_OK;
}

int pa_jacobi_end(pa_ctx* c, pa_report* out) {
  if (int rc = pa_require_solve(c, PA_SOLVE_JACOBI, "pa_jacobi_end")) return rc;
  pa_report tmp;
  int rc = pa_report_read(c, out ? out : &tmp);   // synchronises: itr sweeps were executed
  c->solve = PA_SOLVE_NONE;
  if (rc) return rc;
  // the final iterate lives in the buffer the last EXECUTED sweep wrote (x after an even number of sweeps), the one
  // before it (Field.VARo on request) in the other buffer
  const size_t fb = (size_t)c->G.ncell * (size_t)c->esize;
  void* buf[2] = {c->cg_x, c->scr[SCR_D0]};
  const int fin = (int)(c->h_sc->itr & 1);
  if (c->x_old_out && c->h_sc->itr >= 1)
    PA_HIP(c, hipMemcpyAsync(c->x_old_out, buf[fin ^ 1], fb, hipMemcpyDeviceToDevice, c->stream));
  if (fin) PA_HIP(c, hipMemcpyAsync(c->cg_x, buf[1], fb, hipMemcpyDeviceToDevice, c->stream));
  PA_HIP(c, hipStreamSynchronize(c->stream));
  return (out && out->status) ? PA_E_NONFINITE : PA_OK;
}

}  // extern "C"
