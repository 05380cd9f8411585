// pa_bicgstab.hip -- BiCGSTAB (linalg.py:162-279): the generic kernels, the x / r update, the one-shot driver
// (pa_bicgstab) and the stepwise form on a slab.
#include "pa_solver.h"

// ---- BiCGSTAB kernels (linalg.py:162-279) ------------------------------------------------
// p' = r + beta (p - omega v) (with neighbours, so A p' needs no second pass); v' = A p' on S;
// partial sum r0.v'
template <typename T>
struct BicgPAcc {
  Vec<T> r, p, v;
  T beta, omega;
  __device__ __forceinline__ T at(const DevGeom& G, int64_t i, int64_t j, int64_t k) const {
    const int64_t o = j * G.s1 + k;  // pointers first, one load per field after (see DirAcc)
    const T* rb = r.p + i * G.s0;
    const T* pb = p.p + i * G.s0;
    const T* vb = v.p + i * G.s0;
    if (i < 0) { rb = r.glo; pb = p.glo; vb = v.glo; }
    if (i >= G.n0) { rb = r.ghi; pb = p.ghi; vb = v.ghi; }
    const T rv = rb[o], pv = pb[o], vv = vb[o];
    T t = omega * vv;
    t = pv - t;
    t = beta * t;
    return rv + t;
  }
};

template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_bicg_pv(DevGeom G, DevEq<T> E, const SolverScalars* __restrict__ sc,
                                                       Vec<T> rv, Vec<T> pv, Vec<T> vv, const T* __restrict__ r0,
                                                       T* __restrict__ pnew, T* __restrict__ vnew,
                                                       double* __restrict__ partials) {
  if (sc->done) return;
  BicgPAcc<T> acc{rv, pv, vv, (T)sc->beta, (T)sc->omega};
  double s[1] = {0.0};
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < G.ncell;
       idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t i, j, k;
    pa_decode(G, idx, i, j, k);
    T pc = acc.at(G, i, j, k);
    T vn = (T)0;
    if (pa_in_S(G, i, j, k)) {
      vn = pa_apply_terms<T>(G, E, acc, i, j, k, pc);
      T p = r0[idx] * vn;
      s[0] += (double)p;
    }
    pnew[idx] = pc;
    vnew[idx] = vn;
  }
  pa_block_reduce_store<1>(s, partials);
}

// s = r - alpha v ; partial sum |s|^2 (tol = |r - alpha v|, linalg.py:230-233)
template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_bicg_s(DevGeom G, const SolverScalars* __restrict__ sc,
                                                      const T* __restrict__ r, const T* __restrict__ v,
                                                      T* __restrict__ s_out, double* __restrict__ partials) {
  if (sc->done) return;
  const T alpha = (T)sc->alpha;
  double s[1] = {0.0};
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < G.ncell;
       idx += (int64_t)gridDim.x * blockDim.x) {
    T av = alpha * v[idx];
    T sv = r[idx] - av;
    s_out[idx] = sv;
    T p = sv * sv;
    s[0] += (double)p;
  }
  pa_block_reduce_store<1>(s, partials);
}

// t = A s on S ; partial sums t.s, t.t, r0.t
template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_bicg_t(DevGeom G, DevEq<T> E, const SolverScalars* __restrict__ sc,
                                                      Vec<T> sv, const T* __restrict__ r0, T* __restrict__ t_out,
                                                      double* __restrict__ partials) {
  if (sc->done || sc->finished_early) return;
  FieldAcc<T> acc{sv};
  double s[3] = {0.0, 0.0, 0.0};
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < G.ncell;
       idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t i, j, k;
    pa_decode(G, idx, i, j, k);
    T tv = (T)0;
    if (pa_in_S(G, i, j, k)) {
      T sc_ = sv.p[idx];
      tv = pa_apply_terms<T>(G, E, acc, i, j, k, sc_);
      T a = tv * sc_;
      T b = tv * tv;
      T c = r0[idx] * tv;
      s[0] += (double)a;
      s[1] += (double)b;
      s[2] += (double)c;
    }
    t_out[idx] = tv;
  }
  pa_block_reduce_store<3>(s, partials);
}

#ifndef PA_BX_NTP
#define PA_BX_NTP 1   // k_bicg_x PITCHED: non-temporal accesses of the pitched (vector-aligned) arrays, as in the contiguous layout
#endif
#ifndef PA_BX_XU
#define PA_BX_XU 1    // k_bicg_x PITCHED: x in whole vectors at cell-aligned addresses (one 16-byte access for VEC 8- / 4-byte ones)
#endif
#ifndef PA_BX_XNT
#define PA_BX_XNT 1   // ... and those non-temporal
#endif
// early exit: x += alpha p ; otherwise x = x + alpha p + s omega ; r = s - omega t ; |r|^2
// VEC cells per lane and step (16-byte lane accesses where the four arrays allow them: 166 -> 1xx us at 256^3 fp64,
// DESIGN.md section 4; 1: any alignment / cell count)
// PITCHED (odd row lengths, bicg_run_t): p, s, t, r, v, p_next with a row pitch of ps1 cells (a multiple of the
// vector), x contiguous and touched cell by cell; pad cells are written as 0.
// SRV (round 4): s is not read but re-formed from r and v' -- s = r - alpha v', the combine of phase 6, operation for
// operation, so the same bits -- and r is updated IN PLACE: the tiled s / t phase then stores t alone (15 array passes per
// iteration for 16; s_in unused, v_in required).
template <typename T, int VEC, bool PITCHED = false, bool SRV = false>
__global__ void __launch_bounds__(PA_BLOCK) k_bicg_x(DevGeom G, const SolverScalars* __restrict__ sc,
                                                      T* __restrict__ x, const T* p,   // (p_next may be p: in place)
                                                      const T* __restrict__ s_in, const T* __restrict__ t_in,
                                                      T* __restrict__ r, double* __restrict__ partials,
                                                      const double* pre_part, int pre_n, SolverScalars* sc_w,
                                                      const T* v_in, T* p_next, int64_t ps1 = 0) {
  // p_next != null: also the NEXT direction p'' = r_new + beta (p' - omega v') (linalg.py:217) -- beta = rho_next / rho
  // alpha / omega is complete as soon as omega and rho_next = -omega (r0 . t) are (linalg.py:212, 246-247): the p / v
  // phase of the next iteration then reads ONE field with a halo instead of three and stores one instead of two
  // (v' = A p'' from the stored p'', phase 8 of k_cg3d); p'' goes unused when the stop test that follows ends the solve
  const T alpha = (T)sc->alpha;
  T omega;
  int early;
  T beta_n = (T)0;
  const double rho_cur = sc->rho;
  if (pre_n > 0) {
    // folded stop test 1, then omega and rho' (pa_step_bicg_mid on the rows {|s|^2, t.s, t.t, r0.t} of the fused s / t
    // kernel) -- every block on its own, same summation order; block 0 stores
    // (Both launch sites pass sc_w == sc, so a late block may read the early flag, omega and rho' block 0 has already
    // stored.  All three only pass THROUGH the step: the early flag comes back as it went in on the non-finite path alone,
    // where block 0 stored it unchanged and every block returns; omega and rho' when stop test 1 ended the solve, where
    // the look-ahead beta formed from them goes unused (`pn` is false).  Whatever a block uses, it computed from the sums.)
    __shared__ double pre_sm[24];
    const int done_in = sc->done, early_in = sc->finished_early;
    const double tol_lim = sc->tolerance, omega_in = sc->omega, rho_next_in = sc->rho_next;
    double t4[4];
    if (!pa_fold_sums<4, 0>(pre_part, pre_n, 4, 0, nullptr, 0, done_in, pre_sm, t4)) return;
    if (threadIdx.x == 0) {
      const PaBicgMid m = pa_step_bicg_mid<T>(t4[0], t4[1], t4[2], t4[3], tol_lim, early_in, omega_in, rho_next_in);
      pre_sm[16] = m.om.omega;
      pre_sm[17] = m.stop.early ? 1.0 : 0.0;
      pre_sm[18] = m.stop.err ? 1.0 : 0.0;
      // the next beta, as the step that closes the iteration forms it
      pre_sm[19] = (double)pa_step_bicg_beta<T>((T)m.om.rho_next, (T)rho_cur, alpha, (T)m.om.omega);
      if (blockIdx.x == 0) pa_put(sc_w, m);
    }
    __syncthreads();
    if (pre_sm[18] != 0.0) return;
    omega = (T)pre_sm[16];
    early = pre_sm[17] != 0.0;
    beta_n = (T)pre_sm[19];
  } else {
    if (sc->done) return;
    omega = (T)sc->omega;
    early = sc->finished_early;
    beta_n = pa_step_bicg_beta<T>((T)sc->rho_next, (T)rho_cur, alpha, omega);
  }
  const bool pn = p_next != nullptr && !early;
  double s[1] = {0.0};
  typedef T V __attribute__((ext_vector_type(VEC)));
  const unsigned nvr = PITCHED ? (unsigned)(ps1 / VEC) : 1u;   // vectors per pitched row
  const int64_t nvec = PITCHED ? G.n0 * G.n1 * (int64_t)nvr : G.ncell / VEC;   // (VEC > 1 only for ncell % VEC == 0)
  // Traversal (round 4): every block owns ONE contiguous range of vectors and walks it backwards -- the s / t phase before
  // marched its chunks forwards, the v phase after will again, so what was touched last (still in the Infinity Cache) is
  // read first -- and the once-touched streams (x, r, t) move with non-temporal loads / stores.  The bare 5 : 3 mix at
  // 512^3 fp64 (profiles/tools/streammix2.hip): grid-stride 1.78-1.83 ms, contiguous ranges backwards + nt 1.64.
  constexpr bool NT = VEC > 1 && (!PITCHED || PA_BX_NTP);
  typedef T VU __attribute__((ext_vector_type(VEC), aligned(sizeof(T))));   // PITCHED: a vector of x at a cell-aligned address
  const int64_t per = ((nvec + gridDim.x - 1) / gridDim.x + PA_BLOCK - 1) / PA_BLOCK * PA_BLOCK;
  const int64_t b0 = (int64_t)blockIdx.x * per, b1 = b0 + per < nvec ? b0 + per : nvec;
  auto ldnt = [](const T* q, int64_t i) -> V {
    return NT ? __builtin_nontemporal_load(reinterpret_cast<const V*>(q) + i) : reinterpret_cast<const V*>(q)[i];
  };
  for (int64_t st = b1 > b0 ? (b1 - b0 + PA_BLOCK - 1) / PA_BLOCK - 1 : -1; st >= 0; --st) {
    const int64_t iv = b0 + st * PA_BLOCK + threadIdx.x;
    if (iv >= b1) continue;
    // (p and v' are read here for the last time in the iteration as well: non-temporal, which leaves the Infinity Cache to
    // the p'' this kernel writes for the v phase -- 256^3 fp64, eight interleaved pairs: 0.356-0.379 -> 0.351-0.353 ms / iteration)
    const V pv = ldnt(p, iv);
    V xv;
    T* xrow = nullptr;      // PITCHED: the cells of this vector in the caller's contiguous x
    int nval = VEC;         // ... and how many of them are real cells
    if (PITCHED) {
      const unsigned row = (unsigned)iv / nvr;
      const int64_t col = (int64_t)((unsigned)iv - row * nvr) * VEC;
      if (col >= G.n2) continue;   // a vector of pad cells: zero since the start of the solve, stays zero
      xrow = x + (int64_t)row * G.n2 + col;
      nval = (int)(G.n2 - col < VEC ? G.n2 - col : VEC);
      if (PA_BX_XU && VEC > 1 && nval == VEC) {
        xv = PA_BX_XNT ? __builtin_nontemporal_load(reinterpret_cast<const VU*>(xrow)) : *reinterpret_cast<const VU*>(xrow);
      } else {
#pragma unroll
        for (int v = 0; v < VEC; ++v) xv[v] = v < nval ? xrow[v] : (T)0;
      }
    } else {
      xv = ldnt(x, iv);
    }
    V xn, rn, sv, tv, vv, pq;
    if (!early) {
      if (SRV) {
        const V ro = ldnt(r, iv);
        vv = ldnt(v_in, iv);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          T av = alpha * vv[v];
          sv[v] = ro[v] - av;
        }
      } else {
        sv = reinterpret_cast<const V*>(s_in)[iv];
      }
      tv = ldnt(t_in, iv);
    }
    if (pn && !SRV) vv = ldnt(v_in, iv);
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      T ap = alpha * pv[v];
      T xq = xv[v] + ap;
      if (!early) {
        T so = sv[v] * omega;
        xq = xq + so;
        T ot = omega * tv[v];
        T rq = sv[v] - ot;
        rn[v] = rq;
        T q = rq * rq;
        s[0] += (double)q;
        if (pn) {   // combine of k_cg3d phase 5
          T tq = omega * vv[v];
          tq = pv[v] - tq;
          tq = beta_n * tq;
          pq[v] = rq + tq;
          if (PITCHED && v >= nval) pq[v] = (T)0;
        }
      }
      xn[v] = xq;
    }
    if (pn) reinterpret_cast<V*>(p_next)[iv] = pq;
    if (!early) {
      if (NT) __builtin_nontemporal_store(rn, reinterpret_cast<V*>(r) + iv); else reinterpret_cast<V*>(r)[iv] = rn;
    }
    if (PITCHED) {
      if (PA_BX_XU && VEC > 1 && nval == VEC) {
        if (PA_BX_XNT) __builtin_nontemporal_store((VU)xn, reinterpret_cast<VU*>(xrow));
        else *reinterpret_cast<VU*>(xrow) = xn;
      } else {
#pragma unroll
        for (int v = 0; v < VEC; ++v)
          if (v < nval) xrow[v] = xn[v];
      }
    } else if (NT) {
      __builtin_nontemporal_store(xn, reinterpret_cast<V*>(x) + iv);
    } else {
      reinterpret_cast<V*>(x)[iv] = xn;
    }
  }
  pa_block_reduce_store<1>(s, partials);
}

// The single-block scalar steps (pa_scalar_steps.h).  step 0: alpha, after p / v; 1: stop test 1, after s; 2: omega and
// rho', after t; 12: both, after the fused s / t kernel (rows {|s|^2, t.s, t.t, r0.t}); 3: the close, after x / r;
// 10: the start of a slab solve (rho' = r0.r0, the first beta).  partials non-null: the step's sums are reduced from
// nblk partial rows first; null (slabs): they are the all-reduced entries of `sums` (layout: the slab section below).
template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_bicg_post(SolverScalars* sc, const double* partials, int nblk,
                                                         const double* sums, int step) {
  __shared__ double sm[PA_BLOCK / 64];
  if (step == 10) {
    if (threadIdx.x == 0) {
      pa_logic_bicg_start<T>(sc, sums[1]);
      sc->done = 0;   // `while not finished`: at least one iteration
    }
    return;
  }
  if (sc->done) return;
  const int ncol = step == 2 ? 3 : (step == 12 ? 4 : 1), off = step == 0 ? 0 : (step == 3 ? 5 : (step == 2 ? 2 : 1));
  double v[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (q >= ncol) continue;
    if (partials) v[q] = pa_reduce_partials(partials, nblk, ncol, q, sm);
    else if (threadIdx.x == 0) v[q] = sums[off + q];
  }
  if (threadIdx.x != 0) return;
  if (step == 0) pa_logic_bicg_alpha<T>(sc, v[0]);
  else if (step == 1) pa_logic_bicg_stop1<T>(sc, v[0]);
  else if (step == 2) pa_logic_bicg_omega<T>(sc, v[0], v[1], v[2]);
  else if (step == 12) pa_logic_bicg_mid<T>(sc, v[0], v[1], v[2], v[3]);
  else pa_logic_bicg_close<T>(sc, v[0]);
}

template <typename T>
static int bicg_run_t(pa_ctx* c, T* x, const T* rhs, double tol, int64_t max_it, pa_report* out) {
  const DevGeom& G = c->G;
  if (c->slab) { pa_set_err(c, "pa_bicgstab is single-GPU only in this build"); return PA_E_ARG; }
  int rc;
  if (try_resident<T>(c, 2, x, rhs, tol, max_it, 1.0, out, &rc)) return rc;
  const int nblk = pa_grid_blocks(G.ncell);
  // odd row lengths (round 3): ALL eight solver arrays are the ctx's, so all of them take the PITCH layout
  // (solver_pitch) and the tiled phases keep their 16-byte lanes; only the x / r update touches the caller's x.
  // (an index of vectors must fit 31 bits in k_bicg_x)
  // Measured (us / iteration, one-cell-per-lane -> pitched, same box): 257^3 fp64 498-503 -> 470 (256^3: 430), 2-D 4097^2
  // 574 -> 503, 1025^2 59 -> 50, 129^3 76 -> 78; 257^3 fp32 274 -> 287 -- so: fp64, or a 2-D mesh.
  c->cg_ps1 = (sizeof(T) == 8 || c->ndim == 2) ? solver_pitch<T>(c, x) : 0;
  if (c->cg_ps1 > 0 && G.n0 * G.n1 * (c->cg_ps1 / (16 / (int64_t)sizeof(T))) >= ((int64_t)1 << 31)) c->cg_ps1 = 0;
  c->cg_pitch = c->cg_ps1 > 0 ? 1 : 0;
  struct PitchOff { pa_ctx* c; ~PitchOff() { c->cg_pitch = 0; c->cg_ps1 = 0; } } pitch_off{c};   // (a CG solve sets its own)
  const size_t fb = c->cg_pitch ? (size_t)G.n0 * G.n1 * c->cg_ps1 * sizeof(T) : (size_t)G.ncell * sizeof(T);
  const int ids[] = {SCR_R, SCR_D0, SCR_D1, SCR_R0, SCR_V0, SCR_V1, SCR_S, SCR_TT};
  for (int id : ids)
    if ((rc = pa_scratch(c, &c->scr[id], &c->cap[id], fb))) return rc;
  if ((rc = pa_scratch(c, &c->scr[SCR_PART], &c->cap[SCR_PART], (size_t)PA_MAX_PARTIALS * 6 * sizeof(double)))) return rc;
  if ((rc = init_scalars(c, tol, max_it))) return rc;
  DevEq<T> E;
  pa_build_eq<T>(c, c->nterms, c->terms, E);
  if ((rc = pa_bc_apply_faces<T>(c, x))) return rc;
  T* r = (T*)c->scr[SCR_R];
  T* r0 = (T*)c->scr[SCR_R0];
  T* p[2] = {(T*)c->scr[SCR_D0], (T*)c->scr[SCR_D1]};
  T* v[2] = {(T*)c->scr[SCR_V0], (T*)c->scr[SCR_V1]};
  T* s = (T*)c->scr[SCR_S];
  T* t = (T*)c->scr[SCR_TT];
  double* part = (double*)c->scr[SCR_PART];
  Vec<T> xv = pa_vec_self<T>(c, x);
  // a field of the solver as the tiled phases see it (wrap-around planes of a pitched array: its own)
  auto vec_of = [&](const T* q) -> Vec<T> {
    Vec<T> w = pa_vec_self<T>(c, q);
    if (c->cg_pitch) { w.glo = q + (G.n0 - 1) * G.n1 * c->cg_ps1; w.ghi = q; }
    return w;
  };
  if (c->cg_pitch) {
    // A x (tiled kernel, contiguous) into t, then r0 = r = b - A x scattered into the pitched rows with the loop and
    // partial sums of the contiguous form (k_cg_init, PITCH); pad cells of every array zero for the whole solve
    if ((rc = cg_residual_init_pitch<T>(c, E, xv, rhs, t, r0, r, part))) return rc;
  }
  // the tiled phases do not visit the last boundary row / column of non-periodic axes (launch_cg3d): p, v, s, t are 0
  // there by definition and have to be 0 in every buffer the phases write into (and in the pad cells of pitched rows)
  for (T* q : {p[1], v[1], s, t}) PA_HIP(c, hipMemsetAsync(q, 0, fb, c->stream));
  if (!c->cg_pitch && (rc = cg_residual_init<T>(c, E, xv, rhs, r0, r, (T*)nullptr, (T*)nullptr, part))) return rc;
  PA_HIP(c, hipMemsetAsync(p[0], 0, fb, c->stream));
  PA_HIP(c, hipMemsetAsync(v[0], 0, fb, c->stream));
  // rho_next = sum r0.r0 ; tol0 = sqrt(rho_next) ; first beta = rho_next / 1 * 1 / 1 (linalg.py:201-212)
  launch_post_init<T>(c, part, nblk, 2);
  if ((rc = read_scalars(c))) return rc;
  {
    SolverScalars h = *c->h_sc;
    pa_logic_bicg_start<T>(&h, h.rr);   // (on the host: the square root of tol0 is the host's)
    h.done = 0;  // `while not finished`: at least one iteration
    *c->h_sc = h;
    PA_HIP(c, hipMemcpyAsync(c->sc, c->h_sc, sizeof(h), hipMemcpyHostToDevice, c->stream));
    PA_HIP(c, hipStreamSynchronize(c->stream));
  }
  int cur = 0;
  const int poll = poll_interval(c);
  const bool bicg_static = pa_bc_is_static(c);
  PA_HIP(c, hipEventRecord(c->ev0, c->stream));
  int64_t enq = 0;
  // The three single-block scalar kernels of an iteration are folded into the prologue of the kernel
  // that follows each (pa_cg3d_kernel.h phases 5 / 6, k_bicg_x) when that kernel is a tiled one / the
  // row counts are small; each producer has its own region of SCR_PART, because its consumer reads the
  // rows while writing its own.  `pend*` = rows waiting for a prologue.
  double* const reg0 = part;                                   // r0.v'            (1 column)
  double* const reg1 = part + (size_t)PA_MAX_PARTIALS;         // |s|^2 t.s t.t r0.t (4 columns)
  double* const reg2 = part + 5 * (size_t)PA_MAX_PARTIALS;     // |r|^2            (1 column)
  const bool fold = c->fold && !c->slab;
  int pend3 = 0;
  // the next direction formed by k_bicg_x (one array pass less per iteration, one haloed input instead of three in the
  // p / v phase); option "bicg_pfold" 0: every iteration through the p / v phase, as before round 3
  const bool pfold = c->bicg_pfold != 0;
  bool pgiven = false;
  c->fold_a_n = c->fold_b_n = c->fold_b_nsh = 0;
  if (c->coord == PA_COORD_RZ && pfold && c->fastpath) {
    // Axisymmetric mesh: the only tiled form of the p / v phase is the one that takes p' as given (k_cg2d<..., RZ>, phase
    // 8).  The first iteration has p = v = 0, so its p' = r + beta (0 - omega 0) IS r, bit for bit (linalg.py:189-217):
    // hand phase 8 a copy of r and every iteration -- the first included -- runs on the marching kernel.
    c->plan_only = 1;
    const int v_ok = pa_tile3d_bicg_v<T>(c, E, vec_of(p[0]), (const T*)r0, v[1], reg0);
    c->plan_only = 0;
    (void)hipGetLastError();
    if (v_ok > 0) {
      PA_HIP(c, hipMemcpyAsync(p[0], r, fb, hipMemcpyDeviceToDevice, c->stream));
      pgiven = true;
    }
  }
  if (c->cg_pitch && c->coord == PA_COORD_RZ && !pgiven) { pa_set_err(c, "pitched BiCGSTAB on an axisymmetric mesh needs the marching v phase"); return PA_E_STATE; }
  auto flush3 = [&]() {
    if (pend3 > 0) hipLaunchKernelGGL(k_bicg_post<T>, dim3(1), dim3(PA_BLOCK), 0, c->stream, c->sc, reg2, pend3, (const double*)nullptr, 3);
    pend3 = 0;
    c->fold_b_n = 0;
  };
  PollPipe P;
  bool done = false;
  int64_t batch = 1;
  const int64_t max_enq = std::max<int64_t>(max_it, 1);  // the device stops by itself after max_it iterations
  while (!done) {
    int64_t nb = std::min<int64_t>(batch, max_enq - enq);
    if (nb <= 0) {
      if ((rc = poll_drain(c, P, &done))) return rc;
      if (done) break;
      nb = 1;
    }
   for (int64_t qi = 0; qi < nb; ++qi) {
    Vec<T> rv = vec_of(r), pv = vec_of(p[cur]), vv = vec_of(v[cur]);
    c->fold_b_n = pend3;          // phase 5 closes the previous iteration (and swaps the scalar slots)
    c->fold_b_part = reg2;
    // p' of this iteration: formed by the p / v phase into p[cur ^ 1] -- or already there, in p[cur], left by the
    // previous iteration's k_bicg_x (`pgiven`; tiled kernels only), and the phase is v' = A p' alone
    T* const p_it = pgiven ? p[cur] : p[cur ^ 1];
    int used = pgiven ? pa_tile3d_bicg_v<T>(c, E, pv, (const T*)r0, v[cur ^ 1], reg0)
                      : pa_tile3d_bicg_pv<T>(c, E, rv, pv, vv, (const T*)r0, p[cur ^ 1], v[cur ^ 1], reg0);
    if (used < 0) return used;
    if (pgiven && used == 0) { pa_set_err(c, "pa_bicgstab: the tiled v phase declined in the middle of a solve"); return PA_E_STATE; }
    if (c->cg_pitch && used == 0) { pa_set_err(c, "pitched BiCGSTAB: the tiled p / v phase declined"); return PA_E_STATE; }
    const bool pnext = pfold && used > 0;   // the tiled kernels took this iteration: they take the next one
    if (used > 0) {
      pend3 = 0;
    } else {
      flush3();
      hipLaunchKernelGGL(k_bicg_pv<T>, dim3(nblk), dim3(PA_BLOCK), 0, c->stream, G, E, c->sc, rv, pv, vv, (const T*)r0,
                         p[cur ^ 1], v[cur ^ 1], reg0);
      used = nblk;
    }
    copy_x_old<T>(c, x);   // after the p / v phase: its prologue has decided whether this iteration still runs
    int pend0 = (fold && used <= PA_MAX_GRID) ? used : 0;
    if (!pend0) hipLaunchKernelGGL(k_bicg_post<T>, dim3(1), dim3(PA_BLOCK), 0, c->stream, c->sc, reg0, used, (const double*)nullptr, 0);
    Vec<T> vnv = vec_of(v[cur ^ 1]);
    c->fold_a_n = pend0;          // phase 6 computes alpha itself
    // (option "bicg_srv", default on: the tiled phase stores t alone and k_bicg_x re-forms s from r and v')
    int used2 = pa_tile3d_bicg_st<T>(c, E, rv, vnv, (const T*)r0, c->bicg_srv ? (T*)nullptr : s, t, reg1);
    const bool srv = c->bicg_srv && used2 > 0;
    c->fold_a_n = 0;
    if (used2 < 0) return used2;
    if (c->cg_pitch && used2 == 0) { pa_set_err(c, "pitched BiCGSTAB: the tiled s / t phase declined"); return PA_E_STATE; }
    int pend12 = 0;
    if (used2 > 0) {
      pend12 = (fold && used2 <= PA_MAX_GRID) ? used2 : 0;
      if (!pend12) hipLaunchKernelGGL(k_bicg_post<T>, dim3(1), dim3(PA_BLOCK), 0, c->stream, c->sc, reg1, used2, (const double*)nullptr, 12);
    } else {
      if (pend0) hipLaunchKernelGGL(k_bicg_post<T>, dim3(1), dim3(PA_BLOCK), 0, c->stream, c->sc, reg0, pend0, (const double*)nullptr, 0);
      hipLaunchKernelGGL(k_bicg_s<T>, dim3(nblk), dim3(PA_BLOCK), 0, c->stream, G, c->sc, (const T*)r,
                         (const T*)v[cur ^ 1], s, reg1);
      hipLaunchKernelGGL(k_bicg_post<T>, dim3(1), dim3(PA_BLOCK), 0, c->stream, c->sc, reg1, nblk, (const double*)nullptr, 1);
      Vec<T> sv = pa_vec_self<T>(c, s);
      hipLaunchKernelGGL(k_bicg_t<T>, dim3(nblk), dim3(PA_BLOCK), 0, c->stream, G, E, c->sc, sv, (const T*)r0, t, reg1);
      hipLaunchKernelGGL(k_bicg_post<T>, dim3(1), dim3(PA_BLOCK), 0, c->stream, c->sc, reg1, nblk, (const double*)nullptr, 2);
    }
    {
      constexpr int XV = 16 / (int)sizeof(T);
      const bool vec = G.ncell % XV == 0 && ((((uintptr_t)x | (uintptr_t)p[cur ^ 1] | (uintptr_t)s | (uintptr_t)t | (uintptr_t)r) & 15) == 0);
#define PA_BICG_X(VV, PP, SS, ...)                                                                                          \
      hipLaunchKernelGGL((k_bicg_x<T, VV, PP, SS>), dim3(nblk), dim3(PA_BLOCK), 0, c->stream, G, c->sc, x, (const T*)p_it, \
                         (const T*)s, (const T*)t, r, reg2, (const double*)reg1, pend12, c->sc, (const T*)v[cur ^ 1],      \
                         pnext ? p[cur ^ 1] : (T*)nullptr, ##__VA_ARGS__)
      if (c->cg_pitch) {
        if (srv) PA_BICG_X(XV, true, true, c->cg_ps1); else PA_BICG_X(XV, true, false, c->cg_ps1);
      } else if (vec) {
        if (srv) PA_BICG_X(XV, false, true); else PA_BICG_X(XV, false, false);
      } else {
        if (srv) PA_BICG_X(1, false, true); else PA_BICG_X(1, false, false);
      }
#undef PA_BICG_X
      pgiven = pnext;   // (p[cur ^ 1] is p[cur] of the next iteration; in place when p' came from the p / v phase)
    }
    // Dirichlet faces only: the fill of pa_bicg's set-up stands -- p and s are +-0 on every boundary node, so the x / r
    // update leaves x there as it is (alpha, omega are finite by pa_nan_to_num) and a fill would rewrite the same values
    // (the CG loop skips it the same way): one launch less per iteration, 26 us of 2.9 ms at 512^3, 6 of 40 us at 64^3
    if (!bicg_static && (rc = pa_bc_apply_auto<T>(c, x, true))) return rc;
    if (fold && nblk <= PA_MAX_GRID)
      pend3 = nblk;
    else
      hipLaunchKernelGGL(k_bicg_post<T>, dim3(1), dim3(PA_BLOCK), 0, c->stream, c->sc, reg2, nblk, (const double*)nullptr, 3);
    cur ^= 1;
    ++enq;
   }
    flush3();
    if ((rc = poll_submit(c, P, &done))) return rc;
    batch = std::min<int64_t>(poll, std::max<int64_t>(1, enq));
  }
  if ((rc = read_scalars(c))) return rc;
  return timed_report(c, out);
}

extern "C" int pa_bicgstab(pa_ctx* c, void* x, const void* rhs, double tol, int64_t max_it, pa_report* out) {
  if (!c || !c->grid_set || !c->eq_set) { if (c) pa_set_err(c, "pa_bicgstab: grid/equation not set"); return PA_E_STATE; }
  if (int rc0 = pa_check_eq_applicable(c)) return rc0;
  if (!out) return PA_E_ARG;
  PA_HIP(c, hipSetDevice(c->device));
  return c->dtype == PA_F64 ? bicg_run_t<double>(c, (double*)x, (const double*)rhs, tol, max_it, out)
                            : bicg_run_t<float>(c, (float*)x, (const float*)rhs, tol, max_it, out);
}

// ============================================================================
//  stepwise BiCGSTAB on a slab (linalg.py:162-279 split at its reductions and exchanges)
// ============================================================================
// Config 3 is periodic: CG never meets the reference's stop test there, BiCGSTAB is the solver that
// converges -- so it has to exist on slabs too.  Per iteration, with the planes a rank needs from its axis-0
// neighbours:
//   pv      p' = r + beta (p - omega v) -- on the ghost planes too, from the ghost planes of r, p, v with the owner's
//           recurrence bit for bit, so p is never exchanged -- ; v' = A p' on S ; local sum r0.v'   -> [all-reduce 1]
//                                                                                 -> [exchange the boundary planes of v']
//   st      alpha ; s = r - alpha v' (ghost planes from those of r and v') ; t = A s on S ;
//           local sums |s|^2, t.s, t.t, r0.t                                       -> [all-reduce 4]
//   x       stop test 1, omega, rho' ; x += alpha p' + omega s ; r = s - omega t   -> [exchange r planes (+ periodic x planes)]
//   bc      BC fill of x ; local sum |r|^2                                         -> [all-reduce 1]
//   finish  stop test 2, beta, rho <- rho'
// Two plane exchanges and three small all-reduces per iteration.  The sums travel in the caller's PA_NSUM buffer:
// [0] r0.v', [1] |s|^2 (and r0.r0 of the start), [2] t.s, [3] t.t, [4] r0.t, [5] |r|^2.  Kernels: the tiled phases 5 / 6
// where they apply (they take ghost planes through Vec<T>), else the generic ones; the next direction is NOT folded into
// the x / r update here (its ghost planes would need the new residual's, which is still on the wire).
template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_rows_to_sums(const SolverScalars* __restrict__ sc, const double* __restrict__ partials,
                                                            int nblk, int ncol, double* __restrict__ sums, int off, int guarded) {
  __shared__ double sm[PA_BLOCK / 64];
  if (guarded && sc->done) return;
  for (int q = 0; q < ncol; ++q) {
    const double v = pa_reduce_partials(partials, nblk, ncol, q, sm);
    if (threadIdx.x == 0) sums[off + q] = v;
  }
}

// ghost planes of p' = r + beta (p - omega v): the owner's recurrence (BicgPAcc::at / the combine of phase 5)
template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_ghost_p(const SolverScalars* __restrict__ sc, int64_t n,
                                                       const T* __restrict__ r_lo, const T* __restrict__ r_hi,
                                                       const T* __restrict__ p_lo, const T* __restrict__ p_hi,
                                                       const T* __restrict__ v_lo, const T* __restrict__ v_hi,
                                                       T* __restrict__ o_lo, T* __restrict__ o_hi) {
  if (sc->done) return;
  const T beta = (T)sc->beta, omega = (T)sc->omega;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
    if (r_lo) { T t = omega * v_lo[q]; t = p_lo[q] - t; t = beta * t; o_lo[q] = r_lo[q] + t; }
    if (r_hi) { T t = omega * v_hi[q]; t = p_hi[q] - t; t = beta * t; o_hi[q] = r_hi[q] + t; }
  }
}

// ghost planes of s = r - alpha v' (generic kernels only: the tiled phase 6 forms them on load)
template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_ghost_s(const SolverScalars* __restrict__ sc, int64_t n,
                                                       const T* __restrict__ r_lo, const T* __restrict__ r_hi,
                                                       const T* __restrict__ v_lo, const T* __restrict__ v_hi,
                                                       T* __restrict__ o_lo, T* __restrict__ o_hi) {
  if (sc->done) return;
  const T alpha = (T)sc->alpha;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
    if (r_lo) { T av = alpha * v_lo[q]; o_lo[q] = r_lo[q] - av; }
    if (r_hi) { T av = alpha * v_hi[q]; o_hi[q] = r_hi[q] - av; }
  }
}

namespace {


template <typename T>
int bicg_slab_begin_t(pa_ctx* c, T* x, const T* rhs, double tol, int64_t max_it) {
  const DevGeom& G = c->G;
  const size_t fb = (size_t)G.ncell * sizeof(T), pb = (size_t)G.s0 * sizeof(T);
  const int nblk = pa_grid_blocks(G.ncell);
  int rc;
  c->cg_pitch = 0;
  c->cg_ps1 = 0;
  const int ids[] = {SCR_R, SCR_D0, SCR_D1, SCR_R0, SCR_V0, SCR_V1, SCR_S, SCR_TT};
  for (int id : ids)
    if ((rc = pa_scratch(c, &c->scr[id], &c->cap[id], fb))) return rc;
  if ((rc = pa_scratch(c, &c->scr[SCR_PART], &c->cap[SCR_PART], (size_t)PA_MAX_PARTIALS * 6 * sizeof(double)))) return rc;
  if ((rc = pa_scratch(c, &c->scr[SCR_GHOST], &c->cap[SCR_GHOST], 6 * pb))) return rc;   // p ghosts (lo / hi x ping / pong), s ghosts
  if ((rc = init_scalars(c, tol, max_it))) return rc;
  DevEq<T> E;
  pa_build_eq<T>(c, c->nterms, c->terms, E);
  T* r = (T*)c->scr[SCR_R];
  T* r0 = (T*)c->scr[SCR_R0];
  // (the driver has filled the BCs and exchanged the ghost planes of x: linalg.py:181)
  Vec<T> xv = pa_vec_self<T>(c, x);
  xv.glo = (const T*)c->x_glo;
  xv.ghi = (const T*)c->x_ghi;
  for (int id : {SCR_D0, SCR_D1, SCR_V0, SCR_V1, SCR_S, SCR_TT}) PA_HIP(c, hipMemsetAsync(c->scr[id], 0, fb, c->stream));
  PA_HIP(c, hipMemsetAsync(c->scr[SCR_GHOST], 0, 6 * pb, c->stream));
  // r0 = r = b - A x on S ; local sum r0.r0 ; first / last owned plane of r for the neighbours
  if ((rc = cg_residual_init<T>(c, E, xv, rhs, r0, r, (T*)c->r_send_lo, (T*)c->r_send_hi, (double*)c->scr[SCR_PART]))) return rc;
  hipLaunchKernelGGL(k_rows_to_sums<T>, dim3(1), dim3(PA_BLOCK), 0, c->stream, c->sc, (const double*)c->scr[SCR_PART], nblk, 1,
                     pa_sums(c), 1, 0);
  c->cg_x = x;
  c->cur = 0;
  c->solve = PA_SOLVE_BICG;
  PA_HIP(c, hipGetLastError());
  return PA_OK;
}

template <typename T>
int bicg_slab_pv_t(pa_ctx* c) {
  const DevGeom& G = c->G;
  const int nblk = pa_grid_blocks(G.ncell);
  const size_t pl = (size_t)G.s0;
  DevEq<T> E;
  pa_build_eq<T>(c, c->nterms, c->terms, E);
  T* r = (T*)c->scr[SCR_R];
  T* r0 = (T*)c->scr[SCR_R0];
  T* p[2] = {(T*)c->scr[SCR_D0], (T*)c->scr[SCR_D1]};
  T* v[2] = {(T*)c->scr[SCR_V0], (T*)c->scr[SCR_V1]};
  T* g = (T*)c->scr[SCR_GHOST];
  T* pg_lo[2] = {g, g + 2 * pl};
  T* pg_hi[2] = {g + pl, g + 3 * pl};
  double* part = (double*)c->scr[SCR_PART];
  const int cur = c->cur;
  const bool lo = c->r_recv_lo != nullptr, hi = c->r_recv_hi != nullptr;
  if ((lo && !c->v_recv_lo) || (hi && !c->v_recv_hi)) { pa_set_err(c, "pa_bicg_pv: a neighbour without a receive plane for v (pa_slab_set_v)"); return PA_E_STATE; }
  Vec<T> rv = slab_vec<T>(c, r, c->r_recv_lo, c->r_recv_hi);
  Vec<T> pv = slab_vec<T>(c, p[cur], lo ? pg_lo[cur] : nullptr, hi ? pg_hi[cur] : nullptr);
  Vec<T> vv = slab_vec<T>(c, v[cur], c->v_recv_lo, c->v_recv_hi);
  if (lo || hi)   // the ghost planes of p' for the NEXT iteration (this one forms them on load)
    hipLaunchKernelGGL(k_ghost_p<T>, dim3(pa_grid_blocks(G.s0)), dim3(PA_BLOCK), 0, c->stream, c->sc, G.s0,
                       lo ? (const T*)c->r_recv_lo : nullptr, hi ? (const T*)c->r_recv_hi : nullptr, (const T*)pg_lo[cur],
                       (const T*)pg_hi[cur], (const T*)c->v_recv_lo, (const T*)c->v_recv_hi, pg_lo[cur ^ 1], pg_hi[cur ^ 1]);
  c->fold_a_n = c->fold_b_n = 0;
  int used = pa_tile3d_bicg_pv<T>(c, E, rv, pv, vv, (const T*)r0, p[cur ^ 1], v[cur ^ 1], part);
  if (used < 0) return used;
  if (used == 0) {
    hipLaunchKernelGGL(k_bicg_pv<T>, dim3(nblk), dim3(PA_BLOCK), 0, c->stream, G, E, c->sc, rv, pv, vv, (const T*)r0,
                       p[cur ^ 1], v[cur ^ 1], part);
    used = nblk;
  }
  hipLaunchKernelGGL(k_rows_to_sums<T>, dim3(1), dim3(PA_BLOCK), 0, c->stream, c->sc, (const double*)part, used, 1, pa_sums(c), 0, 1);
  pack_end_planes<T>(c, v[cur ^ 1], c->v_send_lo, c->v_send_hi);
  PA_HIP(c, hipGetLastError());
  return PA_OK;
}

template <typename T>
int bicg_slab_st_t(pa_ctx* c) {
  const DevGeom& G = c->G;
  const int nblk = pa_grid_blocks(G.ncell);
  const size_t pl = (size_t)G.s0;
  DevEq<T> E;
  pa_build_eq<T>(c, c->nterms, c->terms, E);
  T* r = (T*)c->scr[SCR_R];
  T* r0 = (T*)c->scr[SCR_R0];
  T* vn = (T*)c->scr[c->cur ? SCR_V0 : SCR_V1];   // v' of this iteration
  T* s = (T*)c->scr[SCR_S];
  T* t = (T*)c->scr[SCR_TT];
  T* g = (T*)c->scr[SCR_GHOST];
  T* sg_lo = g + 4 * pl;
  T* sg_hi = g + 5 * pl;
  double* part = (double*)c->scr[SCR_PART] + (size_t)PA_MAX_PARTIALS;
  hipLaunchKernelGGL(k_bicg_post<T>, dim3(1), dim3(1), 0, c->stream, c->sc, (const double*)nullptr, 0, (const double*)pa_sums(c), 0);   // alpha, itr
  Vec<T> rv = slab_vec<T>(c, r, c->r_recv_lo, c->r_recv_hi);
  Vec<T> vv = slab_vec<T>(c, vn, c->v_recv_lo, c->v_recv_hi);
  c->fold_a_n = 0;
  // (as on one GPU: the tiled phase stores t alone and the x / r step re-forms s from r and v', option "bicg_srv")
  int used = pa_tile3d_bicg_st<T>(c, E, rv, vv, (const T*)r0, c->bicg_srv ? (T*)nullptr : s, t, part);
  if (used < 0) return used;
  c->bicg_s_stored = (used > 0 && c->bicg_srv) ? 0 : 1;
  if (used > 0) {
    hipLaunchKernelGGL(k_rows_to_sums<T>, dim3(1), dim3(PA_BLOCK), 0, c->stream, c->sc, (const double*)part, used, 4, pa_sums(c), 1, 1);
  } else {
    // generic kernels: s everywhere, its ghost planes, t = A s on S.  (Unlike the one-GPU loop, t is formed even when
    // the first stop test is about to end the solve: the test needs the all-reduced |s|^2, which comes after this call.)
    hipLaunchKernelGGL(k_bicg_s<T>, dim3(nblk), dim3(PA_BLOCK), 0, c->stream, G, c->sc, (const T*)r, (const T*)vn, s, part);
    hipLaunchKernelGGL(k_rows_to_sums<T>, dim3(1), dim3(PA_BLOCK), 0, c->stream, c->sc, (const double*)part, nblk, 1, pa_sums(c), 1, 1);
    const bool lo = c->r_recv_lo != nullptr, hi = c->r_recv_hi != nullptr;
    if (lo || hi)
      hipLaunchKernelGGL(k_ghost_s<T>, dim3(pa_grid_blocks(G.s0)), dim3(PA_BLOCK), 0, c->stream, c->sc, G.s0,
                         lo ? (const T*)c->r_recv_lo : nullptr, hi ? (const T*)c->r_recv_hi : nullptr, (const T*)c->v_recv_lo,
                         (const T*)c->v_recv_hi, sg_lo, sg_hi);
    Vec<T> sv = slab_vec<T>(c, s, lo ? sg_lo : nullptr, hi ? sg_hi : nullptr);
    hipLaunchKernelGGL(k_bicg_t<T>, dim3(nblk), dim3(PA_BLOCK), 0, c->stream, G, E, c->sc, sv, (const T*)r0, t, part);
    hipLaunchKernelGGL(k_rows_to_sums<T>, dim3(1), dim3(PA_BLOCK), 0, c->stream, c->sc, (const double*)part, nblk, 3, pa_sums(c), 2, 1);
  }
  PA_HIP(c, hipGetLastError());
  return PA_OK;
}

template <typename T>
int bicg_slab_x_t(pa_ctx* c) {
  const DevGeom& G = c->G;
  const int nblk = pa_grid_blocks(G.ncell);
  T* x = (T*)c->cg_x;
  T* r = (T*)c->scr[SCR_R];
  T* pn = (T*)c->scr[c->cur ? SCR_D0 : SCR_D1];   // p' of this iteration
  T* s = (T*)c->scr[SCR_S];
  T* t = (T*)c->scr[SCR_TT];
  double* part = (double*)c->scr[SCR_PART] + 5 * (size_t)PA_MAX_PARTIALS;
  hipLaunchKernelGGL(k_bicg_post<T>, dim3(1), dim3(1), 0, c->stream, c->sc, (const double*)nullptr, 0, (const double*)pa_sums(c), 12);   // stop test 1, omega, rho'
  constexpr int XV = 16 / (int)sizeof(T);
  const bool vec = G.ncell % XV == 0 && ((((uintptr_t)x | (uintptr_t)pn | (uintptr_t)s | (uintptr_t)t | (uintptr_t)r) & 15) == 0);
  const T* vn = (const T*)c->scr[c->cur ? SCR_V0 : SCR_V1];   // v' of this iteration (s = r - alpha v' when s was not stored)
#define PA_BICG_XS(VV, SS)                                                                                                        \
  hipLaunchKernelGGL((k_bicg_x<T, VV, false, SS>), dim3(nblk), dim3(PA_BLOCK), 0, c->stream, G, c->sc, x, (const T*)pn, (const T*)s, \
                     (const T*)t, r, part, (const double*)nullptr, 0, c->sc, SS ? vn : (const T*)nullptr, (T*)nullptr)
  if (vec) {
    if (c->bicg_s_stored) PA_BICG_XS(XV, false); else PA_BICG_XS(XV, true);
  } else {
    if (c->bicg_s_stored) PA_BICG_XS(1, false); else PA_BICG_XS(1, true);
  }
#undef PA_BICG_XS
  // what the neighbours need next: the first / last owned plane of the new residual and, on the end ranks of a
  // periodic ring, the x planes the other end's BC fill reads (packed behind them by the driver's buffer layout)
  pack_end_planes<T>(c, r, c->r_send_lo, c->r_send_hi);
  pack_x_planes<T>(c, x);
  PA_HIP(c, hipGetLastError());
  return PA_OK;
}

template <typename T>
int bicg_slab_bc_t(pa_ctx* c) {
  const int nblk = pa_grid_blocks(c->G.ncell);
  int rc = pa_bc_is_static(c) ? PA_OK : pa_bc_apply_auto<T>(c, (T*)c->cg_x, true);   // (Dirichlet faces only: bicg_run_t)
  if (rc) return rc;
  hipLaunchKernelGGL(k_rows_to_sums<T>, dim3(1), dim3(PA_BLOCK), 0, c->stream, c->sc,
                     (const double*)c->scr[SCR_PART] + 5 * (size_t)PA_MAX_PARTIALS, nblk, 1, pa_sums(c), 5, 1);
  PA_HIP(c, hipGetLastError());
  return PA_OK;
}

}  // namespace

extern "C" {

int pa_slab_set_v(pa_ctx* c, void* v_send_lo, void* v_send_hi, const void* v_recv_lo, const void* v_recv_hi) {
  if (!c) return PA_E_ARG;
  if (c->solve != PA_SOLVE_NONE) { pa_set_err(c, "pa_slab_set_v during a solve"); return PA_E_STATE; }
  c->v_send_lo = v_send_lo; c->v_send_hi = v_send_hi;
  c->v_recv_lo = v_recv_lo; c->v_recv_hi = v_recv_hi;
  return PA_OK;
}

int pa_bicg_begin(pa_ctx* c, void* x, const void* rhs, double tol, int64_t max_it) {
  if (!c || !c->grid_set || !c->eq_set) { if (c) pa_set_err(c, "pa_bicg_begin: grid/equation not set"); return PA_E_STATE; }
  if (int rc0 = pa_check_eq_applicable(c)) return rc0;
  if (!c->slab || !c->ext_sums) { pa_set_err(c, "pa_bicg_begin is the stepwise form for slabs (pa_slab_set); one GPU: pa_bicgstab"); return PA_E_STATE; }
  PA_HIP(c, hipSetDevice(c->device));
  return c->dtype == PA_F64 ? bicg_slab_begin_t<double>(c, (double*)x, (const double*)rhs, tol, max_it)
                            : bicg_slab_begin_t<float>(c, (float*)x, (const float*)rhs, tol, max_it);
}

int pa_bicg_start(pa_ctx* c) {   // after the all-reduce of sums[1] = r0.r0
  if (int rc = pa_require_solve(c, PA_SOLVE_BICG, "pa_bicg_start")) return rc;
  if (c->dtype == PA_F64) hipLaunchKernelGGL(k_bicg_post<double>, dim3(1), dim3(1), 0, c->stream, c->sc, (const double*)nullptr, 0, (const double*)pa_sums(c), 10);
  else hipLaunchKernelGGL(k_bicg_post<float>, dim3(1), dim3(1), 0, c->stream, c->sc, (const double*)nullptr, 0, (const double*)pa_sums(c), 10);
  PA_HIP(c, hipGetLastError());
  return PA_OK;
}

int pa_bicg_pv(pa_ctx* c) {
  if (int rc = pa_require_solve(c, PA_SOLVE_BICG, "pa_bicg_pv")) return rc;
  return c->dtype == PA_F64 ? bicg_slab_pv_t<double>(c) : bicg_slab_pv_t<float>(c);
}

int pa_bicg_st(pa_ctx* c) {
  if (int rc = pa_require_solve(c, PA_SOLVE_BICG, "pa_bicg_st")) return rc;
  return c->dtype == PA_F64 ? bicg_slab_st_t<double>(c) : bicg_slab_st_t<float>(c);
}

int pa_bicg_x(pa_ctx* c) {
  if (int rc = pa_require_solve(c, PA_SOLVE_BICG, "pa_bicg_x")) return rc;
  return c->dtype == PA_F64 ? bicg_slab_x_t<double>(c) : bicg_slab_x_t<float>(c);
}

int pa_bicg_bc(pa_ctx* c) {
  if (int rc = pa_require_solve(c, PA_SOLVE_BICG, "pa_bicg_bc")) return rc;
  return c->dtype == PA_F64 ? bicg_slab_bc_t<double>(c) : bicg_slab_bc_t<float>(c);
}

int pa_bicg_finish(pa_ctx* c) {
  if (int rc = pa_require_solve(c, PA_SOLVE_BICG, "pa_bicg_finish")) return rc;
  if (c->dtype == PA_F64) hipLaunchKernelGGL(k_bicg_post<double>, dim3(1), dim3(1), 0, c->stream, c->sc, (const double*)nullptr, 0, (const double*)pa_sums(c), 3);
  else hipLaunchKernelGGL(k_bicg_post<float>, dim3(1), dim3(1), 0, c->stream, c->sc, (const double*)nullptr, 0, (const double*)pa_sums(c), 3);
  c->cur ^= 1;
  PA_HIP(c, hipGetLastError());
  return PA_OK;
}

int pa_bicg_end(pa_ctx* c, pa_report* out) {
  if (int rc = pa_require_solve(c, PA_SOLVE_BICG, "pa_bicg_end")) return rc;
  int rc = out ? pa_report_read(c, out) : PA_OK;
  c->solve = PA_SOLVE_NONE;
  if (rc) return rc;
  return (out && out->status) ? PA_E_NONFINITE : PA_OK;
}

}  // extern "C"
