// pa_scalar_steps.h -- the scalar steps of the solver loops on the device-resident state, each stated ONCE.
//   value level    pa_step_*: operands by value, the result a small struct of plain members (registers after inlining:
//                  a local SolverScalars would put a tiled kernel on scratch memory, ~10 us more per dispatch).  A
//                  member the step leaves alone comes back as it went in, so storing a result is unconditional (pa_put).
//   pointer level  pa_logic_*: a step applied to a SolverScalars* (single-block kernels of pa_cg.hip / pa_bicgstab.hip /
//                  pa_jacobi.hip, the resident solver of pa_resident.hip, whose state sits in LDS).
//   folded         pa_fold_sums / pa_fold_prologue: the step in the prologue of the tiled kernel that follows it
//                  (k_cg3d, k_cg2d; k_bicg_x and k_slab_mid use the reduction).
// Operation order and rounding are the reference's (linalg.py); every function names its lines.
#pragma once
#include "pa_host.h"

template <typename T>
__host__ __device__ __forceinline__ double pa_nan_to_num(T v) {
  return (isnan(v) || isinf(v)) ? 0.0 : (double)v;  // linalg.py:302-305
}

// ---- value level ---------------------------------------------------------------------------------------------------
// the stop test of CG, and the whole step that closes a Jacobi sweep (linalg.py:134, 321-338): a non-finite tol raises
// before the iteration is counted
struct PaStop { double tol; long long itr; int err, done; };
template <typename T>
__host__ __device__ __forceinline__ PaStop pa_step_stop(double dx2, long long itr, long long max_it, double tolerance) {
  const T tol = (T)sqrt(dx2);
  PaStop s = {(double)tol, itr, 0, 0};
  if (isnan(tol) || isinf(tol)) { s.err = 1; s.done = 1; return s; }   // linalg.py:334-336
  s.itr = itr + 1;
  if (s.itr > max_it || !(s.tol > tolerance)) s.done = 1;
  return s;
}

// CG: alpha = r.r / d.Ad (linalg.py:118-120)
struct PaCgAlpha { double dAd, alpha; };
template <typename T>
__host__ __device__ __forceinline__ PaCgAlpha pa_step_cg_alpha(double sum_dAd, double rr) {
  const T dAd = (T)sum_dAd;
  const T a = (T)rr / dAd;
  return {(double)dAd, pa_nan_to_num<T>(a)};
}

// CG: the step that closes an iteration (linalg.py:128-141, 321-338): stop test, then beta = r'.r' / r.r
struct PaCgClose { PaStop stop; double rr_old, beta, rr; };
template <typename T>
__host__ __device__ __forceinline__ PaCgClose pa_step_cg_close(double sum_rr, double dx2, double rr, double rr_old, double beta,
                                                                long long itr, long long max_it, double tolerance) {
  PaCgClose s = {pa_step_stop<T>(dx2, itr, max_it, tolerance), rr_old, beta, rr};
  if (s.stop.err) return s;   // raised before beta
  const T rr_new = (T)sum_rr;
  const T rr_was = (T)rr;
  s.rr_old = (double)rr_was;
  s.beta = (double)(rr_new / rr_was);
  s.rr = (double)rr_new;
  return s;
}

// BiCGSTAB: the next beta = rho' / rho * alpha / omega (linalg.py:212); also k_bicg_x's look-ahead of it
template <typename T>
__host__ __device__ __forceinline__ T pa_step_bicg_beta(T rho_next, T rho, T alpha, T omega) {
  T b = rho_next / rho;
  b = b * alpha;
  b = b / omega;
  return b;
}

// BiCGSTAB: start (linalg.py:201-212): rho' = r0.r0, tol0 = sqrt(rho'), the first beta = rho' / 1 * 1 / 1, rho = rho'
struct PaBicgStart { double rr, rho_next, tol, beta, rho; };
template <typename T>
__host__ __device__ __forceinline__ PaBicgStart pa_step_bicg_start(double sum_r0r0) {
  PaBicgStart s;
  s.rr = (double)(T)sum_r0r0;
  s.rho_next = s.rr;
  s.tol = (double)(T)sqrt((T)s.rr);
  s.beta = (double)pa_step_bicg_beta<T>((T)s.rho_next, (T)1.0, (T)1.0, (T)1.0);
  s.rho = s.rho_next;
  return s;
}

// BiCGSTAB: alpha = rho / (r0 . v') (linalg.py:219-221); the iteration is counted here
struct PaBicgAlpha { double alpha; long long itr; };
template <typename T>
__host__ __device__ __forceinline__ PaBicgAlpha pa_step_bicg_alpha(double sum_r0v, double rho, long long itr) {
  const T r0v = (T)sum_r0v;
  const T rh = (T)rho;
  return {pa_nan_to_num<T>(rh / r0v), itr + 1};
}

// BiCGSTAB: stop test 1 on tol = |s| (linalg.py:230-236)
struct PaBicgStop1 { double tol; int err, early; };
template <typename T>
__host__ __device__ __forceinline__ PaBicgStop1 pa_step_bicg_stop1(double sum_ss, double tolerance, int early) {
  const T tol = (T)sqrt(sum_ss);
  PaBicgStop1 s = {(double)tol, 0, early};
  if (isnan(tol) || isinf(tol)) { s.err = 1; return s; }
  s.early = (s.tol <= tolerance) ? 1 : 0;
  return s;
}

// BiCGSTAB: omega = t.s / t.t, rho' = -omega (r0 . t) (linalg.py:243-247)
struct PaBicgOmega { double omega, rho_next; };
template <typename T>
__host__ __device__ __forceinline__ PaBicgOmega pa_step_bicg_omega(double sum_ts, double sum_tt, double sum_r0t) {
  const T om = (T)pa_nan_to_num<T>((T)sum_ts / (T)sum_tt);
  T rn = -om;
  rn = rn * (T)sum_r0t;
  return {(double)om, (double)rn};
}

// stop test 1, then -- unless it raised or ended the solve -- omega and rho': the two steps above on the four sums of
// the fused s / t phase
struct PaBicgMid { PaBicgStop1 stop; PaBicgOmega om; };
template <typename T>
__host__ __device__ __forceinline__ PaBicgMid pa_step_bicg_mid(double sum_ss, double sum_ts, double sum_tt, double sum_r0t,
                                                                double tolerance, int early, double omega, double rho_next) {
  PaBicgMid s = {pa_step_bicg_stop1<T>(sum_ss, tolerance, early), {omega, rho_next}};
  if (!s.stop.err && !s.stop.early) s.om = pa_step_bicg_omega<T>(sum_ts, sum_tt, sum_r0t);
  return s;
}

// BiCGSTAB: the step that closes an iteration (linalg.py:212-214, 236-262): an early exit skips the second stop test;
// else tol = |r|, the stop tests (`itr >= max_it`, linalg.py:264), the next beta, rho <- rho'
struct PaBicgClose { double tol, beta, rho; int err, done; };
template <typename T>
__host__ __device__ __forceinline__ PaBicgClose pa_step_bicg_close(double sum_rr, int early, double tol, double tolerance,
                                                                    long long itr, long long max_it, double rho_next, double rho,
                                                                    double alpha, double omega, double beta) {
  PaBicgClose s = {tol, beta, rho, 0, 1};
  if (early) return s;
  const T tolv = (T)sqrt(sum_rr);
  s.tol = (double)tolv;
  if (isnan(tolv) || isinf(tolv)) { s.err = 1; return s; }
  s.done = 0;
  if (s.tol <= tolerance) s.done = 1;
  if (itr >= max_it) s.done = 1;
  s.beta = (double)pa_step_bicg_beta<T>((T)rho_next, (T)rho, (T)alpha, (T)omega);
  s.rho = rho_next;
  return s;
}

// ---- a result into the state -----------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ void pa_put(SolverScalars* sc, const PaStop& s) {
  sc->tol = s.tol;
  sc->itr = s.itr;
  if (s.err) sc->err = 1;
  if (s.done) sc->done = 1;
}
__host__ __device__ __forceinline__ void pa_put(SolverScalars* sc, const PaCgAlpha& s) {
  sc->dAd = s.dAd;
  sc->alpha = s.alpha;
}
__host__ __device__ __forceinline__ void pa_put(SolverScalars* sc, const PaCgClose& s) {
  pa_put(sc, s.stop);
  sc->rr_old = s.rr_old;
  sc->beta = s.beta;
  sc->rr = s.rr;
}
__host__ __device__ __forceinline__ void pa_put(SolverScalars* sc, const PaBicgStart& s) {
  sc->rr = s.rr;
  sc->rho_next = s.rho_next;
  sc->tol = s.tol;
  sc->beta = s.beta;
  sc->rho = s.rho;
}
__host__ __device__ __forceinline__ void pa_put(SolverScalars* sc, const PaBicgAlpha& s) {
  sc->itr = s.itr;
  sc->alpha = s.alpha;
}
__host__ __device__ __forceinline__ void pa_put(SolverScalars* sc, const PaBicgStop1& s) {
  sc->tol = s.tol;
  sc->finished_early = s.early;
  if (s.err) { sc->err = 1; sc->done = 1; }
}
__host__ __device__ __forceinline__ void pa_put(SolverScalars* sc, const PaBicgOmega& s) {
  sc->omega = s.omega;
  sc->rho_next = s.rho_next;
}
__host__ __device__ __forceinline__ void pa_put(SolverScalars* sc, const PaBicgMid& s) {
  pa_put(sc, s.stop);
  pa_put(sc, s.om);
}
__host__ __device__ __forceinline__ void pa_put(SolverScalars* sc, const PaBicgClose& s) {
  sc->tol = s.tol;
  sc->beta = s.beta;
  sc->rho = s.rho;
  if (s.err) sc->err = 1;
  if (s.done) sc->done = 1;
}

// ---- pointer level ---------------------------------------------------------------------------------------------------
// CG: sums = {d.Ad, r.r, |dx|^2}
template <typename T>
__device__ __forceinline__ void pa_logic_a(SolverScalars* sc, const double* sums) {
  pa_put(sc, pa_step_cg_alpha<T>(sums[0], sc->rr));
}
template <typename T>
__device__ __forceinline__ void pa_logic_b(SolverScalars* sc, const double* sums) {
  pa_put(sc, pa_step_cg_close<T>(sums[1], sums[2], sc->rr, sc->rr_old, sc->beta, sc->itr, sc->max_it, sc->tolerance));
}
template <typename T>
__device__ __forceinline__ void pa_logic_jacobi(SolverScalars* sc, double dx2) {
  pa_put(sc, pa_step_stop<T>(dx2, sc->itr, sc->max_it, sc->tolerance));
}
template <typename T>
__host__ __device__ __forceinline__ void pa_logic_bicg_start(SolverScalars* sc, double r0r0) {
  pa_put(sc, pa_step_bicg_start<T>(r0r0));
}
template <typename T>
__device__ __forceinline__ void pa_logic_bicg_alpha(SolverScalars* sc, double r0v) {
  pa_put(sc, pa_step_bicg_alpha<T>(r0v, sc->rho, sc->itr));
}
template <typename T>
__device__ __forceinline__ void pa_logic_bicg_stop1(SolverScalars* sc, double ss) {
  pa_put(sc, pa_step_bicg_stop1<T>(ss, sc->tolerance, sc->finished_early));
}
template <typename T>
__device__ __forceinline__ void pa_logic_bicg_omega(SolverScalars* sc, double ts, double tt, double r0t) {
  if (sc->finished_early) return;   // stop test 1 ended the solve: t was not formed
  pa_put(sc, pa_step_bicg_omega<T>(ts, tt, r0t));
}
template <typename T>
__device__ __forceinline__ void pa_logic_bicg_mid(SolverScalars* sc, double ss, double ts, double tt, double r0t) {
  pa_put(sc, pa_step_bicg_mid<T>(ss, ts, tt, r0t, sc->tolerance, sc->finished_early, sc->omega, sc->rho_next));
}
template <typename T>
__device__ __forceinline__ void pa_logic_bicg_close(SolverScalars* sc, double rr) {
  pa_put(sc, pa_step_bicg_close<T>(rr, sc->finished_early, sc->tol, sc->tolerance, sc->itr, sc->max_it, sc->rho_next, sc->rho,
                                   sc->alpha, sc->omega, sc->beta));
}

// ---- folded ----------------------------------------------------------------------------------------------------------
// Every workgroup (256 threads) sums the partial rows the previous kernel left: columns c0 .. c0 + N - 1 of n rows of ns
// doubles and, NSH = 1, nsh shell rows as one more sum (t[N]).  Every load is issued before the first wait and before
// `done` is tested -- one memory round trip (~1-2 us right after a kernel boundary), not one per reduction.  false: the
// solve is over, nothing was summed.  Summation order = pa_reduce_partials, column by column -> the same bits in every
// workgroup and in the single-block kernels; t is valid on thread 0.  sm: 4 * (N + NSH) doubles of LDS.
template <int N, int NSH>
__device__ __forceinline__ bool pa_fold_sums(const double* rows, int n, int ns, int c0, const double* shell, int nsh,
                                             int done, double* sm, double (&t)[N + NSH]) {
  constexpr int M = N + NSH;
  double v[M];
#pragma unroll
  for (int q = 0; q < M; ++q) v[q] = 0.0;
  for (int b = threadIdx.x; b < n; b += 256) {
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] += rows[ns * (int64_t)b + c0 + q];
  }
  if (NSH)
    for (int b = threadIdx.x; b < nsh; b += 256) v[N] += shell[b];
  if (done) return false;
#pragma unroll
  for (int q = 0; q < M; ++q)
    for (int off = 32; off > 0; off >>= 1) v[q] += __shfl_down(v[q], off, 64);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < M; ++q) sm[M * (threadIdx.x >> 6) + q] = v[q];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < M; ++q) t[q] = 0.0;
    for (int w = 0; w < 4; ++w) {
#pragma unroll
      for (int q = 0; q < M; ++q) t[q] += sm[M * w + q];
    }
  }
  return true;
}

// The scalar step a tiled kernel runs in its prologue instead of the single-block kernel before it (A.pre_n > 0; one
// GPU inside pa_cg_iterate / bicg_run_t / the Jacobi loop).  The incoming state is read by value; every workgroup sums
// the rows and its thread 0 runs the step, so all of them get the same bits; what the kernel needs comes back through
// LDS (beta, alpha, omega); workgroup 0 alone stores the state into the slot the launcher named (A.sc_w).  The closing
// steps change `done`, which late workgroups of the same launch still read: their next state goes to the OTHER slot --
// a copy of the incoming one when the solve is already over -- and the launcher swaps the two.  true: the workgroup returns.
enum PaFoldStep { PA_FOLD_CG_CLOSE, PA_FOLD_JACOBI_CLOSE, PA_FOLD_CG_ALPHA, PA_FOLD_BICG_CLOSE, PA_FOLD_BICG_ALPHA };

template <typename T, int STEP, typename Args>
__device__ __forceinline__ bool pa_fold_prologue(const Args& A, double* sm, T& alpha, T& beta, T& omega) {
  constexpr bool CG_CLOSE = STEP == PA_FOLD_CG_CLOSE, JAC_CLOSE = STEP == PA_FOLD_JACOBI_CLOSE;
  constexpr bool CLOSES = CG_CLOSE || JAC_CLOSE || STEP == PA_FOLD_BICG_CLOSE;
  constexpr int N = CG_CLOSE ? 2 : 1, NSH = (CG_CLOSE || JAC_CLOSE) ? 1 : 0;   // rows: {r.r, |dx|^2} + shell, else one column
  const SolverScalars* si = A.sc;
  SolverScalars* so = A.sc_w;
  const int done_in = si->done, early = si->finished_early;
  const double rr = si->rr, rr_old = si->rr_old, beta_in = si->beta, tol_in = si->tol, tolerance = si->tolerance;
  const double rho = si->rho, rho_next = si->rho_next, alpha_in = si->alpha, omega_in = si->omega;
  const long long itr = si->itr, max_it = si->max_it;
  double t[N + NSH];
  if (!pa_fold_sums<N, NSH>(A.pre_part, A.pre_n, NSH ? 2 : 1, JAC_CLOSE ? 1 : 0, A.pre_shell, A.pre_nsh, done_in, sm, t)) {
    if (CLOSES && blockIdx.x == 0 && threadIdx.x == 0) *so = *si;
    return true;
  }
  double* out = sm + 4 * (N + NSH);   // {beta | alpha, done}
  if (threadIdx.x == 0) {
    const bool store = blockIdx.x == 0;
    if constexpr (CG_CLOSE) {
      const PaCgClose s = pa_step_cg_close<T>(t[0], t[1] + t[2], rr, rr_old, beta_in, itr, max_it, tolerance);
      out[0] = s.beta;
      out[1] = s.stop.done ? 1.0 : 0.0;
      if (store) { *so = *si; pa_put(so, s); A.pre_sums[1] = t[0]; A.pre_sums[2] = t[1] + t[2]; }
    } else if constexpr (JAC_CLOSE) {
      const PaStop s = pa_step_stop<T>(t[0] + t[1], itr, max_it, tolerance);
      out[1] = s.done ? 1.0 : 0.0;
      if (store) { *so = *si; pa_put(so, s); A.pre_sums[2] = t[0] + t[1]; }
    } else if constexpr (STEP == PA_FOLD_CG_ALPHA) {
      const PaCgAlpha s = pa_step_cg_alpha<T>(t[0], rr);
      out[0] = s.alpha;
      if (store) { pa_put(so, s); A.pre_sums[0] = t[0]; }
    } else if constexpr (STEP == PA_FOLD_BICG_CLOSE) {
      // (The 152-byte copy is 36 VGPRs while the plane loads of the kernel's own prologue are in flight.  Where it stands
      // decides the register count of the instantiations whose peak is here, and with it their blocks / CU: behind the
      // arithmetic in the CG and Jacobi closes, in front of it in this one -- k_cg3d phase 8, fp32, one cell per lane,
      // 2 rows: 87 VGPRs, 5 blocks / CU as ever; behind, 79 and 6, i.e. another grid and another grouping of the partial sums.
      // That holds for ONE compiler and THIS text: after a change to this function or to the compiler, compare the
      // "blocks/CU" of every launch-log line (PYAPES_HIP_DEBUG) with the library before it: a
      // moved occupancy step changes the bits of tol, and fold 1 against fold 0 of ONE build cannot see that.)
      if (store) *so = *si;
      const PaBicgClose s = pa_step_bicg_close<T>(t[0], early, tol_in, tolerance, itr, max_it, rho_next, rho, alpha_in, omega_in, beta_in);
      out[0] = s.beta;
      out[1] = s.done ? 1.0 : 0.0;
      if (store) pa_put(so, s);
    } else {
      const PaBicgAlpha s = pa_step_bicg_alpha<T>(t[0], rho, itr);
      out[0] = s.alpha;
      if (store) pa_put(so, s);   // (no other workgroup of this launch uses itr)
    }
  }
  __syncthreads();
  if (CLOSES && out[1] != 0.0) return true;
  if (CG_CLOSE || STEP == PA_FOLD_BICG_CLOSE) beta = (T)out[0];
  if (STEP == PA_FOLD_BICG_CLOSE) omega = (T)omega_in;
  if (STEP == PA_FOLD_CG_ALPHA || STEP == PA_FOLD_BICG_ALPHA) alpha = (T)out[0];
  return false;
}
