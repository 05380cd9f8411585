// pa_cg.hip -- CG (linalg.py:33-159): the generic phase kernels, the folded slab "mid" kernel, the one-shot driver
// (pa_cg) and the stepwise entry points (bench.py, the slab-decomposed driver); the tiled phases are pa_cg3d*.hip's.
#include "pa_solver.h"

// ---- CG phase A: d' = r + beta d ; partial sum d'.(A d')  (linalg.py:115-120, 141) ----
template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_cg_a(DevGeom G, DevEq<T> E, const SolverScalars* __restrict__ sc,
                                                    Vec<T> rv, Vec<T> dv, T* __restrict__ dnew,
                                                    double* __restrict__ partials) {
  if (sc->done) return;
  DirAcc<T> acc{rv, dv, (T)sc->beta};
  double s[1] = {0.0};
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < G.ncell;
       idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t i, j, k;
    pa_decode(G, idx, i, j, k);
    T e = (T)0;
    if (pa_in_S(G, i, j, k)) {
      e = acc.at(G, i, j, k);
      T Ad = pa_apply_terms<T>(G, E, acc, i, j, k, e);
      T p = e * Ad;
      s[0] += (double)p;
    }
    dnew[idx] = e;
  }
  pa_block_reduce_store<1>(s, partials);
}

// ---- CG phase B: x += alpha d ; r -= alpha A d ; partial sums r.r and |dx|^2 off-shell
//      (linalg.py:122-134)
template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_cg_b(DevGeom G, DevEq<T> E, const SolverScalars* __restrict__ sc,
                                                    Vec<T> dv, T* __restrict__ x, const T* r, T* r_out,
                                                    T* __restrict__ send_lo, T* __restrict__ send_hi,
                                                    double* __restrict__ partials) {
  if (sc->done) return;
  FieldAcc<T> acc{dv};
  const T alpha = (T)sc->alpha;
  double s[2] = {0.0, 0.0};
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < G.ncell;
       idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t i, j, k;
    pa_decode(G, idx, i, j, k);
    T rn = (T)0;
    if (pa_in_S(G, i, j, k)) {
      T dc = dv.p[idx];
      T Ad = pa_apply_terms<T>(G, E, acc, i, j, k, dc);
      T xo = x[idx];
      T ad = alpha * dc;
      T xn = xo + ad;
      x[idx] = xn;
      T aAd = alpha * Ad;
      rn = r[idx] - aAd;
      T p = rn * rn;
      s[0] += (double)p;
      if (!pa_on_shell(G, i, j, k)) {
        T df = xn - xo;
        T p2 = df * df;
        s[1] += (double)p2;
      }
    }
    // (every node: r itself, or r's new block when the placement search moves it -- 0 outside S, as r is everywhere)
    r_out[idx] = rn;
    if (send_lo && i == 0) send_lo[j * G.s1 + k] = rn;
    if (send_hi && i == G.n0 - 1) send_hi[j * G.s1 + k] = rn;
  }
  pa_block_reduce_store<2>(s, partials);
}

// stage 0: reduce only (multi-GPU, before the all-reduce); 1: logic only; 2: both
template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_cg_post_a(SolverScalars* sc, const double* partials, int nblk,
                                                         double* sums, int stage) {
  __shared__ double sm[PA_BLOCK / 64];
  if (sc->done) return;
  if (stage != 1) {
    double v = pa_reduce_partials(partials, nblk, 1, 0, sm);
    if (threadIdx.x == 0) sums[0] = v;
  }
  if (stage != 0 && threadIdx.x == 0) pa_logic_a<T>(sc, sums);
}

template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_cg_post_b(SolverScalars* sc, const double* partials, int nblk,
                                                         const double* partials_shell, int nblk_shell,
                                                         double* sums, int stage) {
  __shared__ double sm[PA_BLOCK / 64];
  if (sc->done) return;
  if (stage != 1) {
    double rr = pa_reduce_partials(partials, nblk, 2, 0, sm);
    double dx2 = pa_reduce_partials(partials, nblk, 2, 1, sm);
    double sh = nblk_shell > 0 ? pa_reduce_partials(partials_shell, nblk_shell, 1, 0, sm) : 0.0;
    if (threadIdx.x == 0) {
      sums[1] = rr;
      sums[2] = dx2 + sh;
    }
  }
  if (stage != 0 && threadIdx.x == 0) pa_logic_b<T>(sc, sums);
}

// slab: ghost planes of the new direction, d'_g = r_g + beta d_g -- bitwise what the neighbour
// rank computes for its own boundary plane, so no direction planes are ever exchanged
template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_ghost_dir(const SolverScalars* __restrict__ sc, int64_t n,
                                                         const T* __restrict__ r_lo, const T* __restrict__ r_hi,
                                                         const T* __restrict__ d_lo, const T* __restrict__ d_hi,
                                                         T* __restrict__ o_lo, T* __restrict__ o_hi) {
  if (sc->done) return;
  const T beta = (T)sc->beta;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
    if (r_lo) { T b = beta * d_lo[q]; o_lo[q] = r_lo[q] + b; }
    if (r_hi) { T b = beta * d_hi[q]; o_hi[q] = r_hi[q] + b; }
  }
}

// ---- slab, folded iteration: everything between phase A and phase B in ONE launch ------------------
// (i) alpha = r.r / d'.Ad' from the all-reduced d'.Ad' ROWS: every block sums them in the fixed order of
// k_cg_post_a / the phase-B prologue (same bits in every block, block 0 stores the state); (ii) the ghost
// planes of the new direction, d'_g = r_g + beta d_g (k_ghost_dir's recurrence); (iii) the planes the
// neighbours need from this iteration, computed AHEAD of phase B from the same operands in the same order
// (pa_apply_terms' Laplacian branch + k_cg_b's update, which the tiled phase B reproduces bit for bit): the
// new residual on the first / last owned plane and, on the end ranks of a periodic ring, the new x planes
// the other end's BC fill reads.  The packed exchange can therefore start before phase B and fly beside it.
// Folded iterations exist only where the tiled kernels run, i.e. for ONE Laplacian term on an xyz mesh, so
// the stencil is written out with all seven operands loaded up front (one memory round trip per node; the
// generic per-axis evaluation is a chain of three) -- a 512^2 plane pair: 29 us generic, ~10 us like this.
template <typename T>
struct MidArgs {
  const T* d;            // d' of this iteration
  const T* r;            // residual before phase B
  const T* x;            // iterate before phase B
  const T *r_lo, *r_hi;  // ghost planes of r (null: physical end)
  const T *d_lo, *d_hi;  // ghost planes of the PREVIOUS direction
  T *g_lo, *g_hi;        // out: ghost planes of d'
  T *send_lo, *send_hi;  // out: new residual on plane 0 / n0-1
  T *xp_lo1, *xp_hi0, *xp_hi1;  // out (periodic ring ends): new x on plane 1 / n0-1 / n0-2, or null
  LapCoef<T> lap;
  T coeff, sign;
  int has_coeff;
  const T* coeff_f;
};

// one axis of the Laplacian row at global index g: ((cP x+ + cC x) + cM x-), fdc.py:190-198 / pa_apply_terms
template <typename T>
__device__ __forceinline__ T pa_lap_axis(const DevGeom& G, const LapCoef<T>& L, int a, int64_t g, int64_t N, T xp, T xc,
                                         T xm) {
  T cP = L.inv[a], cC = L.m2inv[a], cM = L.inv[a];
  const T cB = L.c23[a];
  const int rc = pa_row_case(G, a, g, N, G.treat);
  if (rc == 1) { cP = cB; cC = -cB; cM = (T)0; }
  if (rc == 2) { cP = (T)0; cC = -cB; cM = cB; }
  return pa_row3<T>(cP, xp, cC, xc, cM, xm);
}

template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_slab_mid(DevGeom G, SolverScalars* sc, const double* __restrict__ rows,
                                                        int nrows, double* __restrict__ sums, MidArgs<T> M) {
  __shared__ double sm[8];
  const int done_in = sc->done;
  const double rr_in = sc->rr;
  const T beta = (T)sc->beta;
  double v[1];
  if (!pa_fold_sums<1, 0>(rows, nrows, 1, 0, nullptr, 0, done_in, sm, v)) return;
  if (threadIdx.x == 0) {
    const PaCgAlpha s = pa_step_cg_alpha<T>(v[0], rr_in);
    sm[4] = s.alpha;
    if (blockIdx.x == 0) {
      pa_put(sc, s);
      sums[0] = v[0];
    }
  }
  __syncthreads();
  const T alpha = (T)sm[4];
  // gridDim.x = 5 sections x nb blocks (sections a rank does not have return at once)
  const int nb = (int)(gridDim.x / 5), sec = (int)(blockIdx.x / nb), bq = (int)(blockIdx.x - sec * nb);
  if (sec == 0 && !M.r_lo) return;
  if (sec == 1 && !M.r_hi) return;
  T* const xout = sec == 2 ? M.xp_lo1 : (sec == 3 ? M.xp_hi0 : M.xp_hi1);
  if (sec >= 2 && !xout) return;
  const int64_t ip = sec == 0 ? 0 : (sec == 1 ? G.n0 - 1 : (sec == 2 ? 1 : (sec == 3 ? G.n0 - 1 : G.n0 - 2)));
  const int64_t gi = ip + G.off0;
  const bool iS = gi >= G.slo[0] && gi <= G.shi[0];
  const T* const dpl = M.d + ip * G.s0;
  for (int64_t q = (int64_t)bq * blockDim.x + threadIdx.x; q < G.s0; q += (int64_t)nb * blockDim.x) {
    int64_t j, k;
    if (G.s0 <= 0x7fffffffLL) {
      const uint32_t qq = (uint32_t)q, s1 = (uint32_t)G.s1, jj = qq / s1;
      j = jj; k = qq - jj * s1;
    } else {
      j = q / G.s1; k = q - j * G.s1;
    }
    const bool inS = iS && j >= G.slo[1] && j <= G.shi[1] && k >= G.slo[2] && k <= G.shi[2];
    const T dc = dpl[q];
    if (sec >= 2) {   // new x on plane 1 / n0-1 / n0-2 (k_cg_b: x + alpha d' on S, x elsewhere)
      const T xo = M.x[ip * G.s0 + q];
      T ad = alpha * dc;
      T xn = xo + ad;
      xout[q] = inS ? xn : xo;
      continue;
    }
    // all operands of the node first: ghost pair, the plane inside, the four in-plane neighbours, r, Gamma
    const T rg = sec == 0 ? M.r_lo[q] : M.r_hi[q];
    const T dg = sec == 0 ? M.d_lo[q] : M.d_hi[q];
    const T din = sec == 0 ? M.d[G.s0 + q] : M.d[(G.n0 - 2) * G.s0 + q];
    const T dj1 = dpl[pa_wrap(j + 1, G.n1) * G.s1 + k], dj0 = dpl[pa_wrap(j - 1, G.n1) * G.s1 + k];
    const T dk1 = dpl[j * G.s1 + pa_wrap(k + 1, G.n2)], dk0 = dpl[j * G.s1 + pa_wrap(k - 1, G.n2)];
    const T rc = M.r[ip * G.s0 + q];
    T cf = M.coeff;
    if (M.has_coeff && M.coeff_f) cf = M.coeff_f[ip * G.s0 + q];
    T bg = beta * dg;
    const T ghost = rg + bg;                 // d'_g = r_g + beta d_g
    if (sec == 0) M.g_lo[q] = ghost; else M.g_hi[q] = ghost;
    // A d' at the node: axes 0 -> 1 -> 2 into zero, * Gamma, * sign, + 0 (pa_apply_terms, kind 0)
    T ax = (T)0;
    ax = ax + pa_lap_axis<T>(G, M.lap, 0, gi, G.g0, sec == 0 ? din : ghost, dc, sec == 0 ? ghost : din);
    ax = ax + pa_lap_axis<T>(G, M.lap, 1, j, G.n1, dj1, dc, dj0);
    ax = ax + pa_lap_axis<T>(G, M.lap, 2, k, G.n2, dk1, dc, dk0);
    if (M.has_coeff) ax = ax * cf;
    ax = ax * M.sign;
    T Ad = (T)0;
    Ad = Ad + ax;
    T aAd = alpha * Ad;
    T rn = rc - aAd;
    rn = inS ? rn : (T)0;
    if (sec == 0) M.send_lo[q] = rn; else M.send_hi[q] = rn;
  }
}

template <typename T>
static int cg_begin_t(pa_ctx* c, T* x, const T* rhs, double tol, int64_t max_it) {
  const DevGeom& G = c->G;
  const size_t fb = (size_t)G.ncell * sizeof(T);
  const int nblk = pa_grid_blocks(G.ncell);
  int rc;
  // odd row lengths: r and the two direction buffers in the PITCH layout (solver_pitch)
  c->cg_ps1 = solver_pitch<T>(c, x);
  c->cg_pitch = c->cg_ps1 > 0 ? 1 : 0;
  const size_t fbp = c->cg_pitch ? (size_t)G.n0 * G.n1 * c->cg_ps1 * sizeof(T) : fb;
  if ((rc = pa_scratch(c, &c->scr[SCR_R], &c->cap[SCR_R], fbp))) return rc;
  if ((rc = pa_scratch(c, &c->scr[SCR_D0], &c->cap[SCR_D0], fbp))) return rc;
  if ((rc = pa_scratch(c, &c->scr[SCR_D1], &c->cap[SCR_D1], fbp))) return rc;
  if ((rc = pa_scratch(c, &c->scr[SCR_PART], &c->cap[SCR_PART], (size_t)PA_MAX_PARTIALS * 4 * sizeof(double)))) return rc;
  if ((rc = pa_scratch(c, &c->scr[SCR_PART2], &c->cap[SCR_PART2], (size_t)3 * PA_MAX_GRID * sizeof(double)))) return rc;
  if ((rc = pa_scratch(c, &c->scr[SCR_SHELL], &c->cap[SCR_SHELL], 2 * (size_t)pa_shell_elems(c) * sizeof(T)))) return rc;
  if ((rc = init_scalars(c, tol, max_it))) return rc;
  // large solves: the online search for the allocations r / d / d' should live in (pa_place.hip) rides on the iterations
  if ((rc = pa_place_begin(c, x, fb))) return rc;   // (before anything is written into r / d)
  // the tiled phase kernels do not visit the last boundary row / column of non-periodic axes: the
  // direction there is 0 by definition and has to be 0 in the buffer the first phase A writes into
  if (!c->cg_pitch) PA_HIP(c, hipMemsetAsync(c->scr[SCR_D1], 0, fb, c->stream));   // (pitched: it first carries A x, below)
  c->cg_x = x;
  c->cur = 0;
  c->fold_a_n = c->fold_b_n = c->fold_b_nsh = 0;  // nothing of an earlier (possibly failed) solve is pending
  c->fold_b_shell = nullptr;
  c->slab_fold = c->slab_fold_live = 0;           // row counts are agreed per solve (pa_cg_fold_plan / _set)
  pa_bc_plan(c);
  c->solve = PA_SOLVE_CG;
  DevEq<T> E;
  pa_build_eq<T>(c, c->nterms, c->terms, E);
  // linalg.py:97.  On a slab the driver fills the BCs itself (pa_apply_bc) BEFORE it exchanges
  // the ghost planes of x, so the fill must not run again here.
  if ((rc = pa_bc_fill_start<T>(c, x, c->slab != 0))) return rc;
  T* r = (T*)c->scr[SCR_R];
  T* d = (T*)c->scr[SCR_D0];
  double* part = (double*)c->scr[SCR_PART];
  Vec<T> xv = pa_vec_self<T>(c, x);
  if (c->slab) { xv.glo = (const T*)c->x_glo; xv.ghi = (const T*)c->x_ghi; }
  if (c->cg_pitch) {
    // A x (tiled kernel, contiguous) into the buffer that becomes the zeroed second direction buffer afterwards
    if ((rc = cg_residual_init_pitch<T>(c, E, xv, rhs, (T*)c->scr[SCR_D1], r, d, part))) return rc;
    PA_HIP(c, hipMemsetAsync(c->scr[SCR_D1], 0, fbp, c->stream));
  }
  if (!c->cg_pitch && (rc = cg_residual_init<T>(c, E, xv, rhs, r, d, (T*)c->r_send_lo, (T*)c->r_send_hi, part))) return rc;
  launch_post_init<T>(c, part, nblk, c->slab ? 0 : 2);
  c->pending_init_logic = c->slab ? 1 : 0;
  if (c->slab) {
    // ghost planes of the two direction buffers: lo/hi x ping/pong, zero = "d = r" with beta = 0
    const size_t pb = (size_t)G.s0 * sizeof(T);
    if ((rc = pa_scratch(c, &c->scr[SCR_GHOST], &c->cap[SCR_GHOST], 4 * pb))) return rc;
    PA_HIP(c, hipMemsetAsync(c->scr[SCR_GHOST], 0, 4 * pb, c->stream));
    char* g = (char*)c->scr[SCR_GHOST];
    c->d_glo[0] = g; c->d_ghi[0] = g + pb; c->d_glo[1] = g + 2 * pb; c->d_ghi[1] = g + 3 * pb;
  }
  PA_HIP(c, hipGetLastError());
  return PA_OK;
}

template <typename T>
static Vec<T> cg_vec(pa_ctx* c, const T* p, int which /*0 r, 1 d cur*/) {
  Vec<T> v = pa_vec_self<T>(c, p);
  if (c->cg_pitch) v.glo = p + (c->G.n0 - 1) * c->G.n1 * c->cg_ps1;   // the wrap-around plane of a pitched array
  if (c->slab) {
    // a NULL recv pointer marks a physical (non-periodic) end: that ghost plane is never used in a
    // result, the field's own plane stands in so that speculative loads stay inside valid memory
    if (which == 0) {
      if (c->r_recv_lo) v.glo = (const T*)c->r_recv_lo;
      if (c->r_recv_hi) v.ghi = (const T*)c->r_recv_hi;
    } else {
      if (c->r_recv_lo) v.glo = (const T*)c->d_glo[c->cur];
      if (c->r_recv_hi) v.ghi = (const T*)c->d_ghi[c->cur];
    }
  }
  return v;
}

// scalar steps that were left to the prologue of a tiled kernel that is not coming (the generic kernel
// runs instead, or the batch of iterations ends): run them as the single-block kernels they replace
template <typename T>
static void cg_flush_fold(pa_ctx* c) {
  if (c->fold_a_n > 0) {
    hipLaunchKernelGGL(k_cg_post_a<T>, dim3(1), dim3(PA_BLOCK), 0, c->stream, c->sc,
                       (const double*)c->scr[SCR_PART] + 2 * (size_t)PA_MAX_PARTIALS, c->fold_a_n, pa_sums(c), 2);
    c->fold_a_n = 0;
  }
  if (c->fold_b_n > 0) {
    hipLaunchKernelGGL(k_cg_post_b<T>, dim3(1), dim3(PA_BLOCK), 0, c->stream, c->sc, c->fold_b_part,
                       c->fold_b_n, c->fold_b_shell ? c->fold_b_shell : (const double*)c->scr[SCR_PART2],
                       c->fold_b_nsh, pa_sums(c), 2);
    c->fold_b_n = c->fold_b_nsh = 0;
    c->fold_b_shell = nullptr;
  }
}

template <typename T>
int pa_cg_phase_a_t(pa_ctx* c, int stage_post) {
  PaRange range_("pyapes CG phase A: d' = r + beta d, sum d'.(A d')");
  const DevGeom& G = c->G;
  const int nblk = pa_grid_blocks(G.ncell);
  DevEq<T> E;
  pa_build_eq<T>(c, c->nterms, c->terms, E);
  T* r = (T*)c->scr[SCR_R];
  T* dold = (T*)c->scr[c->cur ? SCR_D1 : SCR_D0];
  T* dnew = (T*)c->scr[c->cur ? SCR_D0 : SCR_D1];
  double* part = (double*)c->scr[SCR_PART];
  // inside pa_cg_iterate on one GPU the two single-block scalar kernels of an iteration are folded into
  // the prologue of the tiled kernel that follows them (pa_cg3d_kernel.h); d.Ad rows then live in the
  // upper half of SCR_PART, because phase B writes its own rows while its blocks still read these
  const bool foldable = c->fold && c->in_iterate && stage_post == 2 && !c->slab && !c->profile;
  if (foldable) part += 2 * (size_t)PA_MAX_PARTIALS;
  const bool live = c->slab_fold_live != 0;   // folded slab iteration: rows go out through the all-reduce buffer
  if (live) part = c->rows_send;
  if (c->pending_init_logic) {  // slab: sum r.r has been all-reduced by the driver
    launch_post_init<T>(c, nullptr, 0, 1);
    c->pending_init_logic = 0;
  }
  Vec<T> rv = cg_vec<T>(c, r, 0), dv = cg_vec<T>(c, dold, 1);
  if (c->slab && !live && (c->r_recv_lo || c->r_recv_hi)) {
    hipLaunchKernelGGL(k_ghost_dir<T>, dim3(pa_grid_blocks(G.s0)), dim3(PA_BLOCK), 0, c->stream, c->sc, G.s0,
                       (const T*)c->r_recv_lo, (const T*)c->r_recv_hi, (const T*)c->d_glo[c->cur],
                       (const T*)c->d_ghi[c->cur], (T*)c->d_glo[c->cur ^ 1], (T*)c->d_ghi[c->cur ^ 1]);
  }
  if (c->profile) (void)hipEventRecord(c->pev[0], c->stream);
  int rc = pa_cg3d_phase_a<T>(c, E, rv, dv, dnew, part);
  if (rc < 0) return rc;
  int used_blocks = rc;
  if (rc == 0 && live) { pa_set_err(c, "folded slab iteration: the tiled phase A declined after the plan"); return PA_E_STATE; }
  if (rc == 0 && c->cg_pitch) { pa_set_err(c, "pitched CG: the tiled phase A declined"); return PA_E_STATE; }
  if (rc == 0) {
    cg_flush_fold<T>(c);  // the tiled kernel declined: the previous iteration is closed by its own kernel
    hipLaunchKernelGGL(k_cg_a<T>, dim3(nblk), dim3(PA_BLOCK), 0, c->stream, G, E, c->sc, rv, dv, dnew, part);
    used_blocks = nblk;
  }
  if (c->profile) pa_profile_stop(c, 0);
  c->cur ^= 1;
  if (live) {
    // alpha comes from the mid kernel, after the all-reduce of the rows
  } else if (foldable && used_blocks <= PA_MAX_GRID)
    c->fold_a_n = used_blocks;  // phase B's prologue (or cg_flush_fold) computes alpha
  else
    hipLaunchKernelGGL(k_cg_post_a<T>, dim3(1), dim3(PA_BLOCK), 0, c->stream, c->sc, part, used_blocks, pa_sums(c),
                       stage_post);
  PA_HIP(c, hipGetLastError());
  return PA_OK;
}

template <typename T>
int pa_cg_phase_b_t(pa_ctx* c, int stage_post) {
  PaRange range_("pyapes CG phase B: x += alpha d', r -= alpha A d', BC fill, sums");
  const DevGeom& G = c->G;
  const int nblk = pa_grid_blocks(G.ncell);
  DevEq<T> E;
  pa_build_eq<T>(c, c->nterms, c->terms, E);
  T* r = (T*)c->scr[SCR_R];
  T* d = (T*)c->scr[c->cur ? SCR_D1 : SCR_D0];
  T* x = (T*)c->cg_x;
  double* part = (double*)c->scr[SCR_PART];
  double* part2 = (double*)c->scr[SCR_PART2];
  Vec<T> dv = cg_vec<T>(c, d, 1);
  const bool live = c->slab_fold_live != 0;
  if (live) part = c->rows_send + c->fold_rows[0] + c->fold_rows[2];
  if (c->profile) (void)hipEventRecord(c->pev[2], c->stream);
  int rc = pa_cg3d_phase_b<T>(c, E, dv, x, r, part);
  if (rc < 0) return rc;
  int used_blocks = rc;
  if (rc == 0 && live) { pa_set_err(c, "folded slab iteration: the tiled phase B declined after the plan"); return PA_E_STATE; }
  if (rc == 0 && c->cg_pitch) { pa_set_err(c, "pitched CG: the tiled phase B declined"); return PA_E_STATE; }
  if (rc == 0) {
    cg_flush_fold<T>(c);  // alpha by its own kernel
    hipLaunchKernelGGL(k_cg_b<T>, dim3(nblk), dim3(PA_BLOCK), 0, c->stream, G, E, c->sc, dv, x, (const T*)r,
                       c->cg_r_out ? (T*)c->cg_r_out : r, (T*)c->r_send_lo, (T*)c->r_send_hi, part);
    used_blocks = nblk;
  }
  if (c->cg_r_out) pa_place_r_written(c);   // the placement search moved r with this launch: SCR_R is the new block now
  if (c->profile) pa_profile_stop(c, 1);
  c->b_blocks = used_blocks;
  if (c->slab) {  // BC fill + shell + reduction happen in pa_cg_bc, after the driver's plane exchange
    if (!live) pack_x_planes<T>(c, x);
    PA_HIP(c, hipGetLastError());
    return PA_OK;
  }
  int nsh;
  if ((rc = pa_bc_fill_step<T>(c, x, part2, &nsh))) return rc;
  const bool foldable = c->fold && c->in_iterate && stage_post == 2 && !c->slab && !c->profile &&
                        used_blocks <= PA_MAX_GRID && nsh <= 3 * PA_MAX_GRID;
  if (foldable) {
    c->fold_b_n = used_blocks;  // the next phase A's prologue (or cg_flush_fold) closes this iteration
    c->fold_b_nsh = nsh;
    c->fold_b_part = part;
  } else {
    hipLaunchKernelGGL(k_cg_post_b<T>, dim3(1), dim3(PA_BLOCK), 0, c->stream, c->sc, part, used_blocks, part2, nsh,
                       pa_sums(c), stage_post);
  }
  PA_HIP(c, hipGetLastError());
  return PA_OK;
}

// slab: BC fill of x (needs the far planes the driver just exchanged when axis 0 is periodic),
// boundary-shell part of the stop test, local partial sums -> sums[1], sums[2]
template <typename T>
int pa_cg_bc_t(pa_ctx* c) {
  const DevGeom& G = c->G;
  T* x = (T*)c->cg_x;
  double* part = (double*)c->scr[SCR_PART];
  double* part2 = (double*)c->scr[SCR_PART2];
  const bool live = c->slab_fold_live != 0;
  if (live) part2 = c->rows_send + c->fold_rows[0];
  int nsh, rc;
  if ((rc = pa_bc_fill_step<T>(c, x, part2, &nsh))) return rc;
  if (live) {
    // the all-reduced rows are summed by the next phase A's prologue (or pa_cg_slab_flush)
    if (nsh > c->fold_rows[2]) { pa_set_err(c, "folded slab iteration: %d shell rows, %d planned", nsh, c->fold_rows[2]); return PA_E_STATE; }
    c->fold_b_part = c->rows_recv + c->fold_rows[0] + c->fold_rows[2];
    c->fold_b_n = c->fold_rows[1];
    c->fold_b_shell = c->rows_recv + c->fold_rows[0];
    c->fold_b_nsh = c->fold_rows[2];
  } else {
    hipLaunchKernelGGL(k_cg_post_b<T>, dim3(1), dim3(PA_BLOCK), 0, c->stream, c->sc, part, c->b_blocks, part2, nsh,
                       pa_sums(c), 0);
  }
  PA_HIP(c, hipGetLastError());
  return PA_OK;
}

// folded slab iteration, between the all-reduce of the d.Ad rows and phase B (k_slab_mid)
template <typename T>
static int cg_slab_mid_t(pa_ctx* c) {
  const DevGeom& G = c->G;
  DevEq<T> E;
  pa_build_eq<T>(c, c->nterms, c->terms, E);
  if (E.nterms != 1 || E.t[0].kind != PA_OP_LAPLACIAN || c->coord != PA_COORD_XYZ || !G.act[0]) {
    pa_set_err(c, "folded slab iteration: one Laplacian term on a 3-D xyz mesh expected (the tiled kernels' equation)");
    return PA_E_STATE;
  }
  MidArgs<T> M;
  memset(&M, 0, sizeof(M));
  M.lap = E.lap;
  M.coeff = E.t[0].coeff; M.sign = E.t[0].sign; M.has_coeff = E.t[0].has_coeff; M.coeff_f = E.t[0].coeff_f;
  M.d = (const T*)c->scr[c->cur ? SCR_D1 : SCR_D0];
  M.r = (const T*)c->scr[SCR_R];
  M.x = (const T*)c->cg_x;
  M.r_lo = (const T*)c->r_recv_lo; M.r_hi = (const T*)c->r_recv_hi;
  M.d_lo = (const T*)c->d_glo[c->cur ^ 1]; M.d_hi = (const T*)c->d_ghi[c->cur ^ 1];
  M.g_lo = (T*)c->d_glo[c->cur]; M.g_hi = (T*)c->d_ghi[c->cur];
  M.send_lo = (T*)c->r_send_lo; M.send_hi = (T*)c->r_send_hi;
  if ((M.r_lo && !M.send_lo) || (M.r_hi && !M.send_hi)) { pa_set_err(c, "slab: a neighbour without a send plane"); return PA_E_STATE; }
  M.xp_lo1 = (T*)c->x_pack_lo1; M.xp_hi0 = (T*)c->x_pack_hi0; M.xp_hi1 = (T*)c->x_pack_hi1;
  const bool planes = M.r_lo || M.r_hi || M.xp_lo1 || M.xp_hi0 || M.xp_hi1;
  // <= 256 blocks per section: with five sections the whole grid is resident at once (a second round of
  // blocks would pay the prologue's round trip again)
  const int nbm = planes ? std::min(256, pa_grid_blocks(G.s0)) : 1;
  hipLaunchKernelGGL(k_slab_mid<T>, dim3(5 * nbm), dim3(PA_BLOCK), 0, c->stream, G, c->sc,
                     (const double*)c->rows_recv, c->fold_rows[0], pa_sums(c), M);
  PA_HIP(c, hipGetLastError());
  return PA_OK;
}

int pa_cg_slab_mid(pa_ctx* c) {
  return c->dtype == PA_F64 ? cg_slab_mid_t<double>(c) : cg_slab_mid_t<float>(c);
}

int pa_cg_slab_flush(pa_ctx* c) {
  if (c->dtype == PA_F64) cg_flush_fold<double>(c); else cg_flush_fold<float>(c);
  PA_HIP(c, hipGetLastError());
  return PA_OK;
}

template <typename T>
static int cg_run_t(pa_ctx* c, T* x, const T* rhs, double tol, int64_t max_it, pa_report* out) {
  int rc;
  if (try_resident<T>(c, 0, x, rhs, tol, max_it, 1.0, out, &rc)) return rc;
  if ((rc = cg_begin_t<T>(c, x, rhs, tol, max_it))) return rc;
  const int poll = poll_interval(c);
  PA_HIP(c, hipEventRecord(c->ev0, c->stream));
  int64_t enq = 0;
  c->in_iterate = 1;  // scalar steps folded into the next tiled kernel's prologue (flushed before every poll)
  PollPipe P;
  bool done = false;
  int64_t batch = 1;
  while (!done && !rc) {
    // the device stops by itself after max_it + 1 iterations (linalg.py K+1 quirk): never enqueue more
    int64_t nb = std::min<int64_t>(batch, max_it + 1 - enq);
    if (nb <= 0) {
      if ((rc = poll_drain(c, P, &done)) || done) break;
      nb = 1;  // not reached by construction; keeps the loop live if it ever is
    }
    for (int64_t q = 0; q < nb && !rc; ++q) {
      if ((rc = pa_place_tick(c))) break;
      if ((rc = pa_cg_phase_a_t<T>(c, 2))) break;
      copy_x_old<T>(c, x);   // after phase A: its prologue has decided whether this iteration still runs
      rc = pa_cg_phase_b_t<T>(c, 2);
      ++enq;
    }
    if (rc) break;
    if ((rc = pa_place_batch_end(c))) break;
    cg_flush_fold<T>(c);
    rc = poll_submit(c, P, &done);
    batch = std::min<int64_t>(poll, std::max<int64_t>(1, enq));
  }
  if (!rc) rc = read_scalars(c);
  c->in_iterate = 0;
  if (rc) { c->fold_a_n = c->fold_b_n = c->fold_b_nsh = 0; pa_place_end(c, 0); return rc; }
  rc = timed_report(c, out);
  pa_place_end(c, 1);   // (read_scalars has waited for the stream)
  return rc;
}

extern "C" int pa_cg(pa_ctx* c, void* x, const void* rhs, double tol, int64_t max_it, pa_report* out) {
  if (!c || !c->grid_set || !c->eq_set) { if (c) pa_set_err(c, "pa_cg: grid/equation not set"); return PA_E_STATE; }
  if (int rc0 = pa_check_eq_applicable(c)) return rc0;
  if (!out) return PA_E_ARG;
  if (c->slab) { pa_set_err(c, "pa_cg is the single-GPU loop; use the stepwise API on a slab"); return PA_E_STATE; }
  PA_HIP(c, hipSetDevice(c->device));
  const int rc = c->dtype == PA_F64 ? cg_run_t<double>(c, (double*)x, (const double*)rhs, tol, max_it, out)
                                    : cg_run_t<float>(c, (float*)x, (const float*)rhs, tol, max_it, out);
  c->solve = PA_SOLVE_NONE;   // also on the error paths: a failed one-shot solve must not lock the BC / equation state
  pa_place_end(c, 0);
  return rc;
}

// ============================================================================
//  stepwise CG (bench.py, slab-decomposed driver)
// ============================================================================
// rows[0..2] = partial rows this rank's tiled phase A / phase B / BC fill write per iteration (all 0:
// the folded slab sequence does not apply here -- generic kernels, or too many rows)
template <typename T>
static int cg_fold_plan_t(pa_ctx* c, int64_t* rows) {
  rows[0] = rows[1] = rows[2] = 0;
  DevEq<T> E;
  pa_build_eq<T>(c, c->nterms, c->terms, E);
  T* r = (T*)c->scr[SCR_R];
  T* d0 = (T*)c->scr[SCR_D0];
  T* d1 = (T*)c->scr[SCR_D1];
  double* part = (double*)c->scr[SCR_PART];
  c->plan_only = 1;
  const int na = pa_cg3d_phase_a<T>(c, E, cg_vec<T>(c, r, 0), cg_vec<T>(c, d0, 1), d1, part);
  const int nb = pa_cg3d_phase_b<T>(c, E, cg_vec<T>(c, d1, 1), (T*)c->cg_x, r, part);
  c->plan_only = 0;
  (void)hipGetLastError();
  const int ns = c->bc_static ? 0 : pa_bc_shell_rows(c);
  if (na <= 0 || nb <= 0 || na > PA_MAX_GRID || nb > PA_MAX_GRID || ns > 3 * PA_MAX_GRID) return PA_OK;
  rows[0] = na; rows[1] = nb; rows[2] = ns;
  return PA_OK;
}

extern "C" {

int pa_cg_begin(pa_ctx* c, void* x, const void* rhs, double tol, int64_t max_it) {
  if (!c || !c->grid_set || !c->eq_set) { if (c) pa_set_err(c, "pa_cg_begin: grid/equation not set"); return PA_E_STATE; }
  if (int rc0 = pa_check_eq_applicable(c)) return rc0;
  PA_HIP(c, hipSetDevice(c->device));
  return c->dtype == PA_F64 ? cg_begin_t<double>(c, (double*)x, (const double*)rhs, tol, max_it)
                            : cg_begin_t<float>(c, (float*)x, (const float*)rhs, tol, max_it);
}

int pa_cg_phase_a(pa_ctx* c) {
  if (int rc = pa_require_solve(c, PA_SOLVE_CG, "pa_cg_phase_a")) return rc;
  const int st = c->slab ? 0 : 2;
  return c->dtype == PA_F64 ? pa_cg_phase_a_t<double>(c, st) : pa_cg_phase_a_t<float>(c, st);
}

int pa_cg_phase_b(pa_ctx* c) {
  if (int rc = pa_require_solve(c, PA_SOLVE_CG, "pa_cg_phase_b")) return rc;
  if (c->slab && !c->slab_fold_live) {  // alpha from the all-reduced sum d.Ad
    if (c->dtype == PA_F64)
      hipLaunchKernelGGL(k_cg_post_a<double>, dim3(1), dim3(PA_BLOCK), 0, c->stream, c->sc, (const double*)nullptr, 0, pa_sums(c), 1);
    else
      hipLaunchKernelGGL(k_cg_post_a<float>, dim3(1), dim3(PA_BLOCK), 0, c->stream, c->sc, (const double*)nullptr, 0, pa_sums(c), 1);
  }
  const int st = c->slab ? 0 : 2;
  return c->dtype == PA_F64 ? pa_cg_phase_b_t<double>(c, st) : pa_cg_phase_b_t<float>(c, st);
}

int pa_cg_bc(pa_ctx* c) {
  if (int rc = pa_require_solve(c, PA_SOLVE_CG, "pa_cg_bc")) return rc;
  if (!c->slab) return PA_OK;  // done inside phase_b
  return c->dtype == PA_F64 ? pa_cg_bc_t<double>(c) : pa_cg_bc_t<float>(c);
}

int pa_cg_finish_iter(pa_ctx* c) {
  if (int rc = pa_require_solve(c, PA_SOLVE_CG, "pa_cg_finish_iter")) return rc;
  if (!c->slab || c->slab_fold_live) return PA_OK;  // logic already ran inside phase_b / runs in the next prologue
  if (c->dtype == PA_F64)
    hipLaunchKernelGGL(k_cg_post_b<double>, dim3(1), dim3(PA_BLOCK), 0, c->stream, c->sc, (const double*)nullptr, 0,
                       (const double*)nullptr, 0, pa_sums(c), 1);
  else
    hipLaunchKernelGGL(k_cg_post_b<float>, dim3(1), dim3(PA_BLOCK), 0, c->stream, c->sc, (const double*)nullptr, 0,
                       (const double*)nullptr, 0, pa_sums(c), 1);
  PA_HIP(c, hipGetLastError());
  return PA_OK;
}

int pa_cg_fold_plan(pa_ctx* c, int64_t* rows) {
  if (!c || !rows) return PA_E_ARG;
  if (int rc = pa_require_solve(c, PA_SOLVE_CG, "pa_cg_fold_plan")) return rc;
  if (!c->slab) { pa_set_err(c, "pa_cg_fold_plan needs a live slab solve (pa_slab_set, pa_cg_begin)"); return PA_E_STATE; }
  return c->dtype == PA_F64 ? cg_fold_plan_t<double>(c, rows) : cg_fold_plan_t<float>(c, rows);
}

int pa_cg_fold_set(pa_ctx* c, const int64_t* rows) {
  if (!c) return PA_E_ARG;
  if (int rc = pa_require_solve(c, PA_SOLVE_CG, "pa_cg_fold_set")) return rc;
  if (!c->slab) { pa_set_err(c, "pa_cg_fold_set needs a live slab solve"); return PA_E_STATE; }
  c->slab_fold = 0;
  if (!rows || rows[0] <= 0 || rows[1] <= 0 || rows[2] < 0) return PA_OK;   // stepwise sequence
  if (rows[0] > PA_MAX_GRID || rows[1] > PA_MAX_GRID || rows[2] > 3 * PA_MAX_GRID) {
    pa_set_err(c, "pa_cg_fold_set: row counts beyond one resident wave of workgroups");
    return PA_E_ARG;
  }
  int64_t mine[3];
  if (int rc = pa_cg_fold_plan(c, mine)) return rc;
  if (mine[0] <= 0 || mine[0] > rows[0] || mine[1] > rows[1] || mine[2] > rows[2]) {
    pa_set_err(c, "pa_cg_fold_set: agreed rows (%lld %lld %lld) below this rank's (%lld %lld %lld)", (long long)rows[0],
               (long long)rows[1], (long long)rows[2], (long long)mine[0], (long long)mine[1], (long long)mine[2]);
    return PA_E_ARG;
  }
  const size_t tot = (size_t)rows[0] + 2 * (size_t)rows[1] + (size_t)rows[2];
  PA_HIP(c, hipSetDevice(c->device));
  if (tot > c->rows_cap) {
    if (c->rows_buf[0]) (void)hipFree(c->rows_buf[0]);
    if (c->rows_buf[1]) (void)hipFree(c->rows_buf[1]);
    c->rows_buf[0] = c->rows_buf[1] = nullptr;
    c->rows_cap = 0;
    PA_HIP(c, hipMalloc((void**)&c->rows_buf[0], tot * sizeof(double)));
    PA_HIP(c, hipMalloc((void**)&c->rows_buf[1], tot * sizeof(double)));
    c->rows_cap = tot;
  }
  // Rows beyond this rank's own grids are never written: they must be (and stay) zero in the send buffer,
  // hence the all-reduce out of place.  A rank whose counts ARE the agreed ones rewrites every row in every
  // iteration and reduces in place (a local choice: RCCL does not care whether send == recv on a rank).
  c->rows_send = c->rows_buf[0];
  c->rows_recv = (mine[0] == rows[0] && mine[1] == rows[1] && mine[2] == rows[2]) ? c->rows_buf[0] : c->rows_buf[1];
  PA_HIP(c, hipMemsetAsync(c->rows_buf[0], 0, tot * sizeof(double), c->stream));
  PA_HIP(c, hipMemsetAsync(c->rows_buf[1], 0, tot * sizeof(double), c->stream));
  for (int q = 0; q < 3; ++q) c->fold_rows[q] = (int)rows[q];
  c->slab_fold = 1;
  return PA_OK;
}

int pa_cg_iterate(pa_ctx* c, int64_t n) {
  if (int rc = pa_require_solve(c, PA_SOLVE_CG, "pa_cg_iterate")) return rc;
  if (c->slab) { pa_set_err(c, "pa_cg_iterate is single-rank; drive the phases on a slab"); return PA_E_STATE; }
  c->in_iterate = 1;
  int rc = PA_OK;
  for (int64_t q = 0; q < n && !rc; ++q) {
    if ((rc = pa_place_tick(c))) break;
    rc = c->dtype == PA_F64 ? pa_cg_phase_a_t<double>(c, 2) : pa_cg_phase_a_t<float>(c, 2);
    if (!rc) rc = c->dtype == PA_F64 ? pa_cg_phase_b_t<double>(c, 2) : pa_cg_phase_b_t<float>(c, 2);
  }
  c->in_iterate = 0;
  if (!rc) rc = pa_place_batch_end(c);
  if (c->dtype == PA_F64) cg_flush_fold<double>(c); else cg_flush_fold<float>(c);  // the last iteration's stop test
  return rc;
}

int pa_cg_end(pa_ctx* c, pa_report* out) {
  if (int rc = pa_require_solve(c, PA_SOLVE_CG, "pa_cg_end")) return rc;
  int rc = out ? pa_report_read(c, out) : PA_OK;
  c->solve = PA_SOLVE_NONE;
  pa_place_end(c, out ? 1 : 0);   // (pa_report_read has waited for the stream)
  if (rc) return rc;
  return (out && out->status) ? PA_E_NONFINITE : PA_OK;
}

}  // extern "C"
