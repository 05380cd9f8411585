// pa_march.hip -- the explicit march: the generic Euler step / Runge-Kutta stage kernel, ONE step routine (step_t) that
// every entry point goes through, ONE buffer rotation (march_t) that every march is a callable of, and the pa_euler_* /
// pa_rk_* / pa_momentum_march entry points and their forms with a diffusivity field (pa_step_nu, pa_march_nu,
// pa_momentum_march_nu).  The tiled kernels (pa_sf*.hip, pa_sfq*.hip, pa_sfn.hip) take over where they apply.
#include "pa_host.h"

#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <type_traits>

// ---- explicit Euler step [new, SURVEY a15] ----------------------------------------------
// STG: the stage of an SSP Runge-Kutta step (pa_rk_stage) -- the value the Euler step stores, v, leaves as
// c0 * phi0 + c1 * v, the two products and the sum rounded one by one; phi0 is read at the cell.
template <typename T, bool STG> struct EulerStage {};
template <typename T> struct EulerStage<T, true> { const T* phi0; T c0, c1; };
// SRC: the source term (pa_*_src) -- a = nu lap - adv; a = a + s; a = dt a, with s read at the cell on the interior set, or
// the scalar source; the instantiations without it are the code they were
template <typename T, bool SRC> struct EulerSrc {};
template <typename T> struct EulerSrc<T, true> { const T* f; T val; };
// VEL: a velocity, one advection speed per INTERNAL axis (pa_*_vel) -- the advection term is pa_adv_vel below, Eadv is not
// read; the instantiations without it are the code they were
template <typename T, bool VEL> struct EulerVel {};
template <typename T> struct EulerVel<T, true> { const T* f[3]; T val[3]; int kind; };

// NU: a diffusivity field (pa_*_nu) -- the conservative term div(nu grad phi) of pa_nu_term below stands where nu * lap stood,
// Elap's rows and the scalar nu are not read; the instantiations without it are the code they were
template <typename T, bool NU> struct EulerNu {};
template <typename T> struct EulerNu<T, true> { const T* f; T w[3]; };

// d = (+0) + t_0 + t_1 + t_2 over the active axes, nu averaged onto the two faces of axis a (the 1/2 sits in w_a):
//   nup = nu[+1] + nu;  num = nu + nu[-1];  fp = x[+1] - x;  fm = x - x[-1];  t = nup*fp;  s = num*fm;  t = t - s;  t = t * w_a
// with w_a = 0.5 * (ih_a * ih_a), ih_a = fl(1 / dx_a), formed on the host in T.  Neighbours wrap around on every axis; nu is read
// at every node the stencil touches, boundary nodes included, and x through the BC-filled face values (no Neumann 2/3 rows).
template <typename T>
__device__ __forceinline__ T pa_nu_term(const DevGeom& G, const EulerNu<T, true>& D, const FieldAcc<T>& acc, int64_t i, int64_t j,
                                        int64_t k, T xc) {
  const T nc = D.f[i * G.s0 + j * G.s1 + k];
  T d = (T)0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!G.act[a]) continue;
    T xp, xm;
    pa_nbrs<T>(G, acc, a, i, j, k, xp, xm);
    int64_t ii = i, jj = j, kk = k, i2 = i, j2 = j, k2 = k;
    if (a == 0) { ii = pa_wrap(i + 1, G.n0); i2 = pa_wrap(i - 1, G.n0); }
    if (a == 1) { jj = pa_wrap(j + 1, G.n1); j2 = pa_wrap(j - 1, G.n1); }
    if (a == 2) { kk = pa_wrap(k + 1, G.n2); k2 = pa_wrap(k - 1, G.n2); }
    T nup = D.f[ii * G.s0 + jj * G.s1 + kk] + nc;
    T num = nc + D.f[i2 * G.s0 + j2 * G.s1 + k2];
    T fp = xp - xc;
    T fm = xc - xm;
    T t = nup * fp;
    T s = num * fm;
    t = t - s;
    t = t * D.w[a];
    d = d + t;
  }
  return d;
}

// adv = (+0) + t_0 + t_1 + t_2 over the active axes: the per-axis term of pa_apply_terms' scheme `kind` (central, QUICK,
// minmod / mc, upwind), operation for operation -- the central row through pa_central_row / pa_row3, the rest written out as
// there.  What differs: axis a's own speed W.f[a] / W.val[a] stands in the place of the one speed, and there is no rz row.
// TVD: W.kind may be PA_OP_DIV_MINMOD / _MC (k_euler's TVD instantiations); without it that branch is not compiled
template <typename T, bool TVD = false>
__device__ __forceinline__ T pa_adv_vel(const DevGeom& G, const GradCoef<T>& grd, const EulerVel<T, true>& W, const FieldAcc<T>& acc,
                                        int64_t i, int64_t j, int64_t k, T xc) {
  int64_t g[3], N[3];
  pa_gidx(G, i, j, k, g, N);
  const int64_t o = i * G.s0 + j * G.s1 + k;
  T ax = (T)0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!G.act[a]) continue;
    const T* uf = W.f[a];
    const T ucen = uf ? uf[o] : W.val[a];
    T xp, xm;
    pa_nbrs<T>(G, acc, a, i, j, k, xp, xm);
    if (W.kind == 2) {   // PA_OP_DIV_CENTRAL: u_a at the axis's own two neighbours (wrap-around, no slabs here)
      T up = ucen, um = ucen;
      if (uf) {
        int64_t ii = i, jj = j, kk = k, i2 = i, j2 = j, k2 = k;
        if (a == 0) { ii = pa_wrap(i + 1, G.n0); i2 = pa_wrap(i - 1, G.n0); }
        if (a == 1) { jj = pa_wrap(j + 1, G.n1); j2 = pa_wrap(j - 1, G.n1); }
        if (a == 2) { kk = pa_wrap(k + 1, G.n2); k2 = pa_wrap(k - 1, G.n2); }
        up = uf[ii * G.s0 + jj * G.s1 + kk];
        um = uf[i2 * G.s0 + j2 * G.s1 + k2];
      }
      T cP, cC = (T)0 * ucen, cM;
      pa_central_row<T>(G, a, g[a], N[a], up, um, grd.h2[a], cP, cC, cM);
      ax = ax + pa_row3<T>(cP, xp, cC, xc, cM, xm);
    } else {
      const T upl = ucen < (T)0 ? (T)0 : ucen;
      const T umi = ucen > (T)0 ? (T)0 : ucen;
      if (W.kind == 5) {   // PA_OP_DIV_QUICK
        T xpp, xmm;
        pa_nbrs2<T>(G, acc, a, i, j, k, xpp, xmm);
        const bool per = G.bct[2 * a] == 4 || G.bct[2 * a + 1] == 4;
        T cen = xp - xm;
        cen = (T)0.5 * cen;
        T tq = xp + xc;
        tq = (T)0.375 * tq;
        T sq = (T)0.875 * xm;
        tq = tq - sq;
        sq = (T)0.125 * xmm;
        T bq = tq + sq;
        if (!per && g[a] <= 1) bq = cen;
        tq = xm + xc;
        tq = (T)0.375 * tq;
        sq = (T)0.875 * xp;
        tq = sq - tq;
        sq = (T)0.125 * xpp;
        T fq = tq - sq;
        if (!per && g[a] >= N[a] - 2) fq = cen;
        T s = upl * bq;
        T m = umi * fq;
        s = s + m;
        s = s * grd.ih[a];
        ax = ax + s;
      } else if (TVD && (W.kind == 6 || W.kind == 7)) {   // PA_OP_DIV_MINMOD / PA_OP_DIV_MC
        T xpp, xmm;
        pa_nbrs2<T>(G, acc, a, i, j, k, xpp, xmm);
        const bool per = G.bct[2 * a] == 4 || G.bct[2 * a + 1] == 4;
        T bq, fq;
        pa_tvd_halves<T>(xmm, xm, xc, xp, xpp, !per && g[a] <= 1, !per && g[a] >= N[a] - 2, W.kind, bq, fq);
        T s = upl * bq;
        T m = umi * fq;
        s = s + m;
        s = s * grd.ih[a];
        ax = ax + s;
      } else {             // PA_OP_DIV_UPWIND
        T bwd = xc - xm;
        T fwd = xp - xc;
        T s = upl * bwd;
        T m = umi * fwd;
        s = s + m;
        s = s * grd.ih[a];
        ax = ax + s;
      }
    }
  }
  return ax;
}

// TVD: the advection term is a slope-limited scheme, PA_OP_DIV_MINMOD / _MC (pa_device.h pa_tvd_halves) -- instantiations of
// their own, so that the kernels of every other scheme are the code they were
template <typename T, bool STG = false, bool SRC = false, bool VEL = false, bool TVD = false, bool NU = false>
__global__ void __launch_bounds__(PA_BLOCK) k_euler(DevGeom G, DevEq<T> Elap, DevEq<T> Eadv, Vec<T> pv,
                                                     T* __restrict__ out, T nu, T dt, EulerStage<T, STG> S = {},
                                                     EulerSrc<T, SRC> Q = {}, EulerVel<T, VEL> W = {}, EulerNu<T, NU> D = {}) {
  FieldAcc<T> acc{pv};
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < G.ncell;
       idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t i, j, k;
    pa_decode(G, idx, i, j, k);
    T pc = pv.p[idx];
    T v = pc;
    if (pa_in_S(G, i, j, k)) {
      T lap;
      if constexpr (NU) lap = pa_nu_term<T>(G, D, acc, i, j, k, pc);
      else lap = pa_apply_terms<T>(G, Elap, acc, i, j, k, pc);
      T adv;
      if constexpr (VEL) adv = pa_adv_vel<T, TVD>(G, Elap.grd, W, acc, i, j, k, pc);
      else adv = pa_apply_terms<T, TVD>(G, Eadv, acc, i, j, k, pc);
      T a;
      if constexpr (NU) a = lap;   // the diffusivity is inside the term
      else a = nu * lap;
      a = a - adv;
      if constexpr (SRC) {
        const T s = Q.f ? Q.f[idx] : Q.val;
        a = a + s;
      }
      a = dt * a;
      v = pc + a;
    }
    if constexpr (STG) {
      T t0 = S.c0 * S.phi0[idx];
      T t1 = S.c1 * v;
      v = t0 + t1;
    }
    out[idx] = v;
  }
}

// the stage where it cannot be fused (a periodic face, step_t): x <- c0 * phi0 + c1 * x, x the finished Euler step
template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_rk_combine(T* __restrict__ x, const T* __restrict__ phi0, T c0, T c1, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    T t0 = c0 * phi0[i];
    T t1 = c1 * x[i];
    x[i] = t0 + t1;
  }
}

// ---- one step routine ---------------------------------------------------------------------------
// what step_t answers, besides PA_OK and an error, when the BC-on-load form was asked for and does not apply: nothing was launched
#define PA_STEP_DECLINED 1

// PYAPES_HIP_DEBUG: one line per path taken, `budget` of them per print site (the tests read and count these lines)
static bool step_dbg(int* left, int budget) {
  if (*left < 0) *left = getenv("PYAPES_HIP_DEBUG") ? budget : 0;
  if (*left <= 0) return false;
  --*left;
  return true;
}

// The Euler step or the fused stage, in -> out, on the path that takes it: a tiled kernel (pa_tile3d_step: k_sfq, k_sf, k_cg3d),
// else the generic k_euler; then the ordered BC fill.  bcl: the "BC on load" form of a march
// (pa_sf_kernel.h) -- the step kernel alone, no fill behind it, the boundary nodes of `out` stay whatever they were; the answer is
// PA_STEP_DECLINED when that form does not apply here.  nuf: the diffusivity field (pa_*_nu) -- div(nu grad phi) in the place of
// nu * lap, `nu` is not read; never with bcl.
template <typename T>
static int step_t(pa_ctx* c, const T* in, T* out, const StepAdv& adv, double nu, double dt, const StepStage<T>& stage,
                  const pa_source* src, bool bcl = false, const void* nuf = nullptr) {
  const T* phi0 = stage.phi0;
  const pa_velocity* vel = adv.vel;
  if (phi0 && !bcl) {
    // A stage combines the Euler STEP, BC fill included.  For dirichlet / neumann / symmetry faces the fill rewrites its
    // nodes from interior-set values alone, so filling once, after the combination, gives the same bits and the stage is
    // one kernel.  The periodic fill is not of that kind: its lower face reads the upper face's value BEFORE the fill
    // rewrites it (bcs.py:253-262: x[0] = x[1] - x[n-1] + x[n-2]), and those nodes belong to the interior set -- B(c0 phi0 +
    // c1 e) would see the raw stencil value there where the Euler step hands on its filled one.  With a periodic face the
    // stage is therefore the step itself, then the combination in place, then the fill.
    bool periodic = false;
    for (int f = 0; f < 6; ++f) periodic = periodic || (c->G.act[f >> 1] && c->bc[f].type == PA_BC_PERIODIC);
    if (periodic) {
      if (int rc = step_t<T>(c, in, out, adv, nu, dt, {nullptr, 0.0, 0.0}, src, false, nuf)) return rc;   // the source enters in the step only
      static int dbg = -1;
      if (!vel && !nuf && step_dbg(&dbg, 8))
        fprintf(stderr, "[pyapes_hip] k_rk_combine (RK stage, periodic face): Euler step, then %lld cells in place\n", (long long)c->G.ncell);
      if (c->profile) (void)hipEventRecord(c->pev[0], c->stream);
      hipLaunchKernelGGL(k_rk_combine<T>, dim3(pa_grid_blocks(c->G.ncell)), dim3(PA_BLOCK), 0, c->stream, out, phi0, (T)stage.c0,
                         (T)stage.c1, c->G.ncell);
      if (c->profile) pa_profile_stop(c, 0);
      PA_HIP(c, hipGetLastError());
      return pa_bc_apply_auto<T>(c, out, false);
    }
  }
  Vec<T> pv = pa_vec_self<T>(c, in);
  if (!vel && !bcl && c->G.n0 != c->G.g0 && c->ndim == 3) {
    // a slab (pyapes_amd/slab.py SlabEuler): ghost planes from pa_slab_set; a NULL one marks a physical end, whose
    // boundary plane no interior node reads across -- the field's own end plane stands in for the speculative loads
    if (!c->slab) { pa_set_err(c, "pa_euler_step on a slab needs pa_slab_set (ghost planes)"); return PA_E_STATE; }
    pv.glo = c->x_glo ? (const T*)c->x_glo : in;
    pv.ghi = c->x_ghi ? (const T*)c->x_ghi : in + (c->G.n0 - 1) * c->G.s0;
  }
  if (c->profile) (void)hipEventRecord(c->pev[0], c->stream);   // slot 0: the step kernel (without its BC fill)
  // the tiled layer first: k_sfq (QUICK, minmod, mc), k_sf, k_cg3d's Euler phase; 0: none of them takes the launch
  // (a source: the SRC instantiations of k_sf / k_sfq or the generic kernel -- k_cg3d's Euler phase takes none)
  const int fr = pa_tile3d_step<T>(c, pv, out, StepRequest<T>{adv, nu, dt, stage, src, bcl, nuf});
  if (fr < 0) return fr;
  if (fr == 0 && bcl) return PA_STEP_DECLINED;
  if (fr == 0) {
    static int dbg_vel = -1, dbg_src = -1, dbg_stg = -1;   // (source, velocity: one budget for every mesh and both forms, larger than an instantiation's 8)
    const long long nc = (long long)c->G.ncell;
    static int dbg_nu = -1;
    if (nuf) {
      if (step_dbg(&dbg_nu, 64))
        fprintf(stderr, "[pyapes_hip] k_euler%s%s%s (diffusivity field): generic kernel, %lld cells\n", phi0 ? " (RK stage)" : "", src ? " (source)" : "",
                vel ? " (velocity)" : "", nc);
    } else if (vel) {
      if (step_dbg(&dbg_vel, 64)) fprintf(stderr, "[pyapes_hip] k_euler%s%s (velocity): generic kernel, %lld cells\n", phi0 ? " (RK stage)" : "", src ? " (source)" : "", nc);
    } else if (src) {
      if (step_dbg(&dbg_src, 64)) fprintf(stderr, "[pyapes_hip] k_euler%s (source): generic kernel, %lld cells\n", phi0 ? " (RK stage)" : "", nc);
    } else if (phi0) {
      if (step_dbg(&dbg_stg, 8)) fprintf(stderr, "[pyapes_hip] k_euler (RK stage): generic kernel, %lld cells\n", nc);
    }
    DevEq<T> El, Ea;
    pa_build_lap<T>(c, El);
    if (!vel) {
      pa_term ta;
      memset(&ta, 0, sizeof(ta));
      ta.kind = adv.kind; ta.sign = 1.0; ta.u = adv.u; ta.u_field = adv.u_field;
      pa_build_eq<T>(c, 1, &ta, Ea);
    }
    with_bool(phi0 != nullptr, [&](auto stg) {
      with_bool(src != nullptr, [&](auto sc) {
        with_bool(vel != nullptr, [&](auto vl) {
         with_bool(adv.kind == PA_OP_DIV_MINMOD || adv.kind == PA_OP_DIV_MC, [&](auto tv) {
          with_bool(nuf != nullptr, [&](auto nf) {
          constexpr bool STG = decltype(stg)::value, SRC = decltype(sc)::value, VEL = decltype(vl)::value, TVD = decltype(tv)::value;
          constexpr bool NU = decltype(nf)::value;
          EulerStage<T, STG> S;
          EulerSrc<T, SRC> Q;
          EulerVel<T, VEL> W;
          EulerNu<T, NU> D;
          if constexpr (NU) {   // w_a = 0.5 * (ih_a * ih_a), each operation rounded in T
            D.f = (const T*)nuf;
            for (int a = 0; a < 3; ++a) {
              T w = El.grd.ih[a] * El.grd.ih[a];
              w = (T)0.5 * w;
              D.w[a] = w;
            }
          }
          if constexpr (STG) S = {phi0, (T)stage.c0, (T)stage.c1};
          if constexpr (SRC) Q = {(const T*)src->field, (T)src->value};
          if constexpr (VEL) {
            for (int a = 0; a < 3; ++a) { W.f[a] = (const T*)vel->field[a]; W.val[a] = (T)vel->value[a]; }
            W.kind = adv.kind;
          }
          // (with a velocity El stands in for Eadv: unread)
          hipLaunchKernelGGL((k_euler<T, STG, SRC, VEL, TVD, NU>), dim3(pa_grid_blocks(c->G.ncell)), dim3(PA_BLOCK), 0, c->stream, c->G,
                             El, VEL ? El : Ea, pv, out, (T)nu, (T)dt, S, Q, W, D);
          });
         });
        });
      });
    });
  }
  if (c->profile) pa_profile_stop(c, 0);
  PA_HIP(c, hipGetLastError());
  // BC on load: no fill.  Slab mode: the step kernel alone -- the fill of a periodic axis 0 reads planes of the NEW field that
  // live on the other end rank of the ring, so the driver exchanges those first and then calls pa_apply_bc itself.
  if (bcl || c->slab) return PA_OK;
  return pa_bc_apply_auto<T>(c, out, false);
}

// ---- one rotation ---------------------------------------------------------------------------------
// nsteps SSP Runge-Kutta steps of `order` over buf[0..2]: per step launch(in, out, null, 0, 0) -- the Euler step -- and then
// order - 1 fused stages launch(in, out, phi0, c0, c1), out = B(c0 phi0 + c1 E(in)).  *final: the buffer that holds the result.
// Order 1 has no fused stage: buf[0] and buf[1] ping-pong, buf[2] is never touched and *final == nsteps & 1.
template <typename T, typename Launch>
static int march_t(T* const buf[3], int order, int64_t nsteps, int* final, Launch&& launch) {
  // the fused stages of a step in Shu-Osher form, after its plain Euler stage: (c0, c1) of c0 phi0 + c1 E(phi_s)
  static const double ssp[4][2][2] = {{}, {}, {{0.5, 0.5}}, {{3.0 / 4.0, 1.0 / 4.0}, {1.0 / 3.0, 2.0 / 3.0}}};
  const double (*st)[2] = ssp[order];
  int base = 0, wa = 1, wb = 2;   // buffer of the step's phi0 and the two free ones
  for (int64_t s = 0; s < nsteps; ++s) {
    if (int rc = launch(buf[base], buf[wa], (const T*)nullptr, 0.0, 0.0)) return rc;
    int cur = wa, free_ = wb;
    for (int q = 0; q < order - 1; ++q) {
      if (int rc = launch(buf[cur], buf[free_], (const T*)buf[base], st[q][0], st[q][1])) return rc;
      std::swap(cur, free_);
    }
    // cur holds the new state; the old base and the other work buffer are free
    const int old = base;
    base = cur; wa = old; wb = free_;
  }
  *final = base;
  return PA_OK;
}

// (QUICK, minmod and mc march with a BC fill per step or stage: kind == PA_OP_DIV_UPWIND below)
// "BC on load" (pa_sf_kernel.h): when every face has a scalar dirichlet / neumann / symmetry BC the steps of a
// march need no fill between them -- each forms the face values it reads from its own operands, bit for bit what
// the fill would have stored -- and ONE ordered fill after the last step completes the result.  (A source term is read on
// the interior set only: it changes nothing here.)
static bool march_bcl_wanted(const pa_ctx* c, int kind, int64_t nsteps) {
  bool bcl = c->bcl && c->sf && !c->slab && c->ndim == 3 && kind == PA_OP_DIV_UPWIND && nsteps >= 2 &&
             c->G.n0 >= 5 && c->G.n1 >= 5 && c->G.n2 >= 5;
  for (int f = 0; f < 6 && bcl; ++f)
    bcl = c->bc[f].type >= PA_BC_DIRICHLET && c->bc[f].type <= PA_BC_SYMMETRY && !c->bc[f].vals;
  return bcl;
}

// One launch of a one-speed march, in -> out.  *bcl: the march is in the "BC on load" form.  The form is decided by the
// first launch (nlaunch 0); should a later one decline it (an operand the vector kernel does not take), `in` gets the
// fill it was left without and the march goes on in the classic sequence -- the same bits, since the face values a
// BC-on-load launch forms are the ones the fill stores.
template <typename T>
static int bcl_launch_t(pa_ctx* c, bool* bcl, int64_t nlaunch, T* in, T* out, const StepAdv& adv, double nu, double dt,
                        const StepStage<T>& stage, const pa_source* src) {
  if (*bcl) {
    const int rc = step_t<T>(c, in, out, adv, nu, dt, stage, src, true);
    if (rc != PA_STEP_DECLINED) return rc;
    *bcl = false;
    if (nlaunch > 0) {
      if (int rc2 = pa_bc_apply_auto<T>(c, in, false)) return rc2;
    }
  }
  return step_t<T>(c, in, out, adv, nu, dt, stage, src);
}

// The marches of a scalar with one speed (pa_euler_march, pa_rk_march) or that advects itself (self, pa_rk_march_self: every
// launch takes its own input buffer as the speed field): step_t through the BC-on-load driver, the one fill after the loop
template <typename T>
static int march_one_t(pa_ctx* c, void* const b[3], int order, int kind, double u, const void* u_field, bool self, double nu,
                       double dt, int64_t nsteps, int* final, const pa_source* src) {
  T* const buf[3] = {(T*)b[0], (T*)b[1], (T*)b[2]};
  bool bcl = march_bcl_wanted(c, kind, nsteps);
  int64_t nl = 0;
  const int rc = march_t<T>(buf, order, nsteps, final, [&](T* in, T* out, const T* phi0, double c0, double c1) {
    return bcl_launch_t<T>(c, &bcl, nl++, in, out, StepAdv{kind, u, self ? in : u_field, nullptr, -1}, nu, dt, {phi0, c0, c1}, src);
  });
  if (rc) return rc;
  return bcl && nsteps > 0 ? pa_bc_apply_auto<T>(c, buf[*final], false) : PA_OK;
}

// pa_rk_march_vel: step_t directly, a BC fill behind every step and stage
template <typename T>
static int march_vel_t(pa_ctx* c, void* const b[3], int order, int kind, const pa_velocity* vel, double nu, double dt,
                       int64_t nsteps, int* final, const pa_source* src) {
  T* const buf[3] = {(T*)b[0], (T*)b[1], (T*)b[2]};
  return march_t<T>(buf, order, nsteps, final, [&](T* in, T* out, const T* phi0, double c0, double c1) {
    return step_t<T>(c, in, out, StepAdv{kind, 0.0, nullptr, vel, -1}, nu, dt, {phi0, c0, c1}, src);
  });
}

// pa_march_nu with a diffusivity field: step_t directly, a BC fill behind every step and stage (there is no BC-on-load form of
// the term).  vel null: one speed, u / u_field, or -- self -- every launch takes its own input buffer as the speed field
template <typename T>
static int march_nu_t(pa_ctx* c, void* const b[3], int order, int kind, double u, const void* u_field, bool self,
                      const pa_velocity* vel, double dt, int64_t nsteps, int* final, const pa_source* src, const void* nuf) {
  T* const buf[3] = {(T*)b[0], (T*)b[1], (T*)b[2]};
  return march_t<T>(buf, order, nsteps, final, [&](T* in, T* out, const T* phi0, double c0, double c1) {
    return step_t<T>(c, in, out, StepAdv{kind, u, self ? (const void*)in : u_field, vel, -1}, 0.0, dt, {phi0, c0, c1}, src, false, nuf);
  });
}

// pa_momentum_march: the rotation over (ncomp, ncell) buffers.  A stage computes every component from the SAME input vector:
// component q of `in` goes to component q of `out` with component q's BC values in the bound list (types, order and dxf stay),
// advected by the frozen velocity `fz` or, fz null, by the input vector itself -- internal axis ia carries component
// ia - (3 - ndim).  The bound list's values are restored on every way out.  nuf: one diffusivity field for every component.
template <typename T>
static int march_momentum_t(pa_ctx* c, void* const b[3], int ncomp, int order, int kind, const pa_velocity* fz, double nu,
                            double dt, int64_t nsteps, int* final, const pa_source* src, const pa_bc_values* bcv,
                            const void* nuf = nullptr) {
  T* const buf[3] = {(T*)b[0], (T*)b[1], (T*)b[2]};
  const int64_t nc = c->G.ncell;
  const int sh = 3 - c->ndim;
  HostBC saved[6];
  for (int f = 0; f < 6; ++f) saved[f] = c->bc[f];
  const int rc = march_t<T>(buf, order, nsteps, final, [&](T* in, T* out, const T* phi0, double c0, double c1) -> int {
    pa_velocity vi;
    if (fz) vi = *fz;
    else {
      memset(&vi, 0, sizeof(vi));
      vi.has = 1;
      for (int a = 0; a < ncomp; ++a) vi.field[a + sh] = in + a * nc;
    }
    for (int q = 0; q < ncomp; ++q) {
      for (int f = 0; f < 2 * c->ndim; ++f) { c->bc[f + 2 * sh].value = bcv[q].value[f]; c->bc[f + 2 * sh].vals = bcv[q].vals[f]; }
      const pa_source* sq = (src && src[q].has) ? &src[q] : nullptr;
      if (int rc = step_t<T>(c, in + q * nc, out + q * nc, StepAdv{kind, 0.0, nullptr, &vi, fz ? -1 : q + sh}, nu, dt,
                             {phi0 ? phi0 + q * nc : nullptr, c0, c1}, sq, false, nuf))
        return rc;
    }
    return PA_OK;
  });
  for (int f = 0; f < 6; ++f) c->bc[f] = saved[f];
  return rc;
}

// ---- the checks of the entry points, made before anything is enqueued -------------------------------------------------
static bool on_slab(const pa_ctx* c) { return c->slab || (c->G.n0 != c->G.g0 && c->ndim == 3); }

// [p, p + pbytes) against the buffers of a call, each `bbytes` long (null entries: not part of the call)
static bool overlaps(const void* p, size_t pbytes, std::initializer_list<const void*> bufs, size_t bbytes) {
  for (const void* b : bufs)
    if (p && b && (const char*)p < (const char*)b + bbytes && (const char*)b < (const char*)p + pbytes) return true;
  return false;
}

static size_t field_bytes(const pa_ctx* c) { return (size_t)c->G.ncell * (c->dtype == PA_F64 ? 8 : 4); }

// a velocity by INTERNAL axis (a d-dimensional mesh occupies the last d internal axes; the others carry a zero speed that is
// never read)
static void velocity_internal(const pa_ctx* c, const pa_velocity* vel, pa_velocity* vi) {
  memset(vi, 0, sizeof(*vi));
  vi->has = 1;
  for (int a = 0; a < c->ndim; ++a) {
    vi->value[a + 3 - c->ndim] = vel->value[a];
    vi->field[a + 3 - c->ndim] = vel->field[a];
  }
}

// The source of a pa_*_src call.  NULL or has == 0: *src becomes null and the call is its sibling.  Else slab mode
// (PA_E_STATE), an axisymmetric mesh and a field that overlaps one of the call's buffers (PA_E_ARG) are refused.
static int check_source(pa_ctx* c, const pa_source** src, const char* who, std::initializer_list<const void*> bufs) {
  if (!*src || !(*src)->has) { *src = nullptr; return PA_OK; }
  if (on_slab(c)) { pa_set_err(c, "%s: a source term is single GPU only (no slabs)", who); return PA_E_STATE; }
  if (c->coord != PA_COORD_XYZ) { pa_set_err(c, "%s: a source term is for xyz meshes (no axisymmetric rows)", who); return PA_E_ARG; }
  if (overlaps((*src)->field, field_bytes(c), bufs, field_bytes(c))) {
    pa_set_err(c, "%s: the source field must not be one of the call's buffers", who);
    return PA_E_ARG;
  }
  return PA_OK;
}

// The velocity of a pa_*_vel call: the refusals of the header, and the velocity by INTERNAL axis in *vi.
static int check_velocity(pa_ctx* c, const pa_velocity* vel, pa_velocity* vi, int kind, const pa_source* src, const char* who,
                          std::initializer_list<const void*> bufs) {
  if (!vel || !vel->has) { pa_set_err(c, "%s: a velocity is needed (vel == NULL or has == 0)", who); return PA_E_ARG; }
  if (kind == PA_OP_DIV_UPWIND_COMPAT) { pa_set_err(c, "%s: the literal upwind form takes no velocity", who); return PA_E_ARG; }
  if (on_slab(c)) { pa_set_err(c, "%s: a velocity is single GPU only (no slabs)", who); return PA_E_STATE; }
  if (c->coord != PA_COORD_XYZ) { pa_set_err(c, "%s: a velocity is for xyz meshes (no axisymmetric rows)", who); return PA_E_ARG; }
  velocity_internal(c, vel, vi);
  const size_t bytes = field_bytes(c);
  for (int a = 0; a < c->ndim; ++a)
    if (overlaps(vel->field[a], bytes, {src ? src->field : nullptr}, bytes) || overlaps(vel->field[a], bytes, bufs, bytes)) {
      pa_set_err(c, "%s: a velocity field must not be one of the call's buffers or the source field", who);
      return PA_E_ARG;
    }
  return PA_OK;
}

// The diffusivity of a pa_*_nu call.  NULL or has == 0: *nuf stays null and the call is its sibling.  Else the refusals of the
// header: a null field, the literal upwind kind, an axisymmetric mesh, a field that overlaps one of the call's buffers, each
// `bbytes` long (PA_E_ARG); slab mode (PA_E_STATE).
static int check_diffusivity(pa_ctx* c, const pa_diffusivity* dif, const void** nuf, int kind, const char* who,
                             std::initializer_list<const void*> bufs, size_t bbytes) {
  *nuf = nullptr;
  if (!dif || !dif->has) return PA_OK;
  if (!dif->field) { pa_set_err(c, "%s: a diffusivity with has != 0 needs its field", who); return PA_E_ARG; }
  if (kind == PA_OP_DIV_UPWIND_COMPAT) { pa_set_err(c, "%s: the literal upwind form takes no diffusivity field", who); return PA_E_ARG; }
  if (on_slab(c)) { pa_set_err(c, "%s: a diffusivity field is single GPU only (no slabs)", who); return PA_E_STATE; }
  if (c->coord != PA_COORD_XYZ) { pa_set_err(c, "%s: a diffusivity field is for xyz meshes (no axisymmetric rows)", who); return PA_E_ARG; }
  if (overlaps(dif->field, field_bytes(c), bufs, bbytes)) {
    pa_set_err(c, "%s: the diffusivity field must not be one of the call's buffers", who);
    return PA_E_ARG;
  }
  *nuf = dif->field;
  return PA_OK;
}

// what an entry point asks of check_march_call beyond the common rules
enum {
  MC_W2_ALWAYS = 1,   // three buffers at every order (pa_rk_march); else order 1 does not look at w2, and *w2 becomes null
  MC_NO_SLAB = 2,     // the stages march on one GPU: a slab is refused, after the buffers
};

// The refusals every march makes first, in the order they have always been made: the context, the order, (ncomp > 0,
// pa_momentum_march: the mesh and the component count,) the Div kind, the buffers / result index / step count -- `need` is the
// sentence that says what is needed -- and the slab.  The buffers of a scalar march must be distinct; those of the vector march
// are (ncomp, ncell) long, and the caller tests them for overlap.
static int check_march_call(pa_ctx* c, const char* who, int order, int kind, const void* phi, const void* w1, void** w2,
                            int64_t nsteps, const int* final, const char* need, int flags, int ncomp = 0) {
  if (!c || !c->grid_set) return PA_E_STATE;
  if (order < 1 || order > 3) { pa_set_err(c, "%s: order %d (1, 2 or 3)", who, order); return PA_E_ARG; }
  if (ncomp) {
    if (on_slab(c)) { pa_set_err(c, "%s: single GPU only (no slabs)", who); return PA_E_STATE; }
    if (c->coord != PA_COORD_XYZ) { pa_set_err(c, "%s: for xyz meshes (no axisymmetric rows)", who); return PA_E_ARG; }
    if (c->ndim < 2 || ncomp != c->ndim) {
      pa_set_err(c, "%s: one component per mesh axis on a 2-D or 3-D mesh (%d components, %d axes)", who, ncomp, c->ndim);
      return PA_E_ARG;
    }
    if (kind == PA_OP_DIV_UPWIND_COMPAT) { pa_set_err(c, "%s: the literal upwind form takes no velocity", who); return PA_E_ARG; }
  }
  if (int rc = pa_check_div_kind(c, kind, who)) return rc;
  if (order == 1 && !(flags & MC_W2_ALWAYS)) *w2 = nullptr;
  const bool three = order > 1 || (flags & MC_W2_ALWAYS);
  bool ok = phi && w1 && final && nsteps >= 0 && (!three || *w2);
  if (!ncomp) ok = ok && phi != w1 && phi != *w2 && w1 != *w2;
  if (!ok) { pa_set_err(c, "%s: %s", who, need); return PA_E_ARG; }
  if ((flags & MC_NO_SLAB) && on_slab(c)) { pa_set_err(c, "%s: single GPU only (no slab stages)", who); return PA_E_STATE; }
  return PA_OK;
}

#define PA_BY_DTYPE(c, fn, ...) ((c)->dtype == PA_F64 ? fn<double>(__VA_ARGS__) : fn<float>(__VA_ARGS__))

// one step or stage (phi0 non-null) in the context's dtype: the single-launch entry points
static int step_any(pa_ctx* c, const void* in, void* out, const StepAdv& adv, double nu, double dt, const void* phi0, double c0,
                    double c1, const pa_source* src, const void* nuf = nullptr) {
  PA_HIP(c, hipSetDevice(c->device));
  return c->dtype == PA_F64 ? step_t<double>(c, (const double*)in, (double*)out, adv, nu, dt, {(const double*)phi0, c0, c1}, src, false, nuf)
                            : step_t<float>(c, (const float*)in, (float*)out, adv, nu, dt, {(const float*)phi0, c0, c1}, src, false, nuf);
}

extern "C" {

int pa_euler_step_vel(pa_ctx* c, const void* in, void* out, int kind, const pa_velocity* vel, double nu, double dt,
                      const pa_source* src) {
  if (!c || !c->grid_set) return PA_E_STATE;
  int rc = pa_check_div_kind(c, kind, "pa_euler_step_vel");
  if (rc) return rc;
  if (!in || !out || in == out) { pa_set_err(c, "pa_euler_step_vel: in-place step is not allowed"); return PA_E_ARG; }
  if ((rc = check_source(c, &src, "pa_euler_step_vel", {in, out}))) return rc;
  pa_velocity vi;
  if ((rc = check_velocity(c, vel, &vi, kind, src, "pa_euler_step_vel", {in, out}))) return rc;
  return step_any(c, in, out, StepAdv{kind, 0.0, nullptr, &vi, -1}, nu, dt, nullptr, 0.0, 0.0, src);
}

int pa_rk_stage_vel(pa_ctx* c, const void* phi, const void* phi0, void* out, double c0, double c1, int kind,
                    const pa_velocity* vel, double nu, double dt, const pa_source* src) {
  if (!c || !c->grid_set) return PA_E_STATE;
  int rc = pa_check_div_kind(c, kind, "pa_rk_stage_vel");
  if (rc) return rc;
  if (!phi || !phi0 || !out || out == phi || out == phi0) {
    pa_set_err(c, "pa_rk_stage_vel: out must be a buffer of its own (not phi, not phi0)");
    return PA_E_ARG;
  }
  if ((rc = check_source(c, &src, "pa_rk_stage_vel", {phi, phi0, out}))) return rc;
  pa_velocity vi;
  if ((rc = check_velocity(c, vel, &vi, kind, src, "pa_rk_stage_vel", {phi, phi0, out}))) return rc;
  return step_any(c, phi, out, StepAdv{kind, 0.0, nullptr, &vi, -1}, nu, dt, phi0, c0, c1, src);
}

int pa_rk_march_vel(pa_ctx* c, void* phi, void* w1, void* w2, int order, int kind, const pa_velocity* vel, double nu,
                    double dt, int64_t nsteps, int* final, const pa_source* src) {
  int rc = check_march_call(c, "pa_rk_march_vel", order, kind, phi, w1, &w2, nsteps, final,
                            "distinct buffers (two for order 1, else three), a place for the result index and nsteps >= 0 are needed", 0);
  if (rc) return rc;
  if ((rc = check_source(c, &src, "pa_rk_march_vel", {phi, w1, w2}))) return rc;
  pa_velocity vi;
  if ((rc = check_velocity(c, vel, &vi, kind, src, "pa_rk_march_vel", {phi, w1, w2}))) return rc;
  PaRange range_("pyapes march in a velocity field");
  PA_HIP(c, hipSetDevice(c->device));
  void* const b[3] = {phi, w1, w2};
  return PA_BY_DTYPE(c, march_vel_t, c, b, order, kind, &vi, nu, dt, nsteps, final, src);
}

int pa_momentum_march(pa_ctx* c, void* U, void* w1, void* w2, int ncomp, int order, int kind, const pa_velocity* frozen, double nu,
                      double dt, int64_t nsteps, int* final, const pa_source* src, const pa_bc_values* bcv) {
  return pa_momentum_march_nu(c, U, w1, w2, ncomp, order, kind, frozen, nu, dt, nsteps, final, src, bcv, nullptr);
}

int pa_momentum_march_nu(pa_ctx* c, void* U, void* w1, void* w2, int ncomp, int order, int kind, const pa_velocity* frozen, double nu,
                         double dt, int64_t nsteps, int* final, const pa_source* src, const pa_bc_values* bcv,
                         const pa_diffusivity* dif) {
  const char* who = (dif && dif->has) ? "pa_momentum_march_nu" : "pa_momentum_march";
  int rc = check_march_call(c, who, order, kind, U, w1, &w2, nsteps, bcv ? final : nullptr,
                            "buffers (two for order 1, else three), a place for the result index, BC values and nsteps >= 0 are needed",
                            0, ncomp);
  if (rc) return rc;
  const size_t cbytes = field_bytes(c), vbytes = cbytes * (size_t)ncomp;
  if (overlaps(U, vbytes, {w1, w2}, vbytes) || overlaps(w1, vbytes, {w2}, vbytes)) {
    pa_set_err(c, "%s: the buffers must not overlap", who);
    return PA_E_ARG;
  }
  pa_velocity vi;
  if (frozen) {
    if (!frozen->has) { pa_set_err(c, "%s: a frozen velocity with has == 0", who); return PA_E_ARG; }
    velocity_internal(c, frozen, &vi);
    for (int a = 0; a < c->ndim; ++a)
      if (overlaps(frozen->field[a], cbytes, {U, w1, w2}, vbytes)) { pa_set_err(c, "%s: a frozen velocity field must not overlap a buffer of the call", who); return PA_E_ARG; }
  }
  if (src)
    for (int q = 0; q < ncomp; ++q)
      if (src[q].has && overlaps(src[q].field, cbytes, {U, w1, w2}, vbytes)) { pa_set_err(c, "%s: a source field must not overlap a buffer of the call", who); return PA_E_ARG; }
  const int64_t n[3] = {c->G.n0, c->G.n1, c->G.n2};
  for (int q = 0; q < ncomp; ++q)
    for (int f = 0; f < 2 * c->ndim; ++f)
      if (overlaps(bcv[q].vals[f], cbytes / (size_t)n[(f >> 1) + 3 - c->ndim], {U, w1, w2}, vbytes)) {
        pa_set_err(c, "%s: a BC face array must not overlap a buffer of the call", who);
        return PA_E_ARG;
      }
  const void* nuf;
  if ((rc = check_diffusivity(c, dif, &nuf, kind, who, {U, w1, w2}, vbytes))) return rc;
  PaRange range_("pyapes momentum march");
  PA_HIP(c, hipSetDevice(c->device));
  void* const b[3] = {U, w1, w2};
  return PA_BY_DTYPE(c, march_momentum_t, c, b, ncomp, order, kind, frozen ? &vi : nullptr, nu, dt, nsteps, final, src, bcv, nuf);
}

int pa_step_nu(pa_ctx* c, const void* phi, const void* phi0, void* out, double c0, double c1, int kind, double u, const void* u_field,
               const pa_velocity* vel, double nu, double dt, const pa_source* src, const pa_diffusivity* dif) {
  if (!dif || !dif->has) {   // the sibling itself
    if (vel) return phi0 ? pa_rk_stage_vel(c, phi, phi0, out, c0, c1, kind, vel, nu, dt, src) : pa_euler_step_vel(c, phi, out, kind, vel, nu, dt, src);
    return phi0 ? pa_rk_stage_src(c, phi, phi0, out, c0, c1, kind, u, u_field, nu, dt, src) : pa_euler_step_src(c, phi, out, kind, u, u_field, nu, dt, src);
  }
  const char* who = "pa_step_nu";
  if (!c || !c->grid_set) return PA_E_STATE;
  int rc = pa_check_div_kind(c, kind, who);
  if (rc) return rc;
  if (!phi || !out || out == phi || out == phi0) {
    pa_set_err(c, "%s: out must be a buffer of its own (not phi, not phi0)", who);
    return PA_E_ARG;
  }
  if ((rc = check_source(c, &src, who, {phi, phi0, out, vel ? nullptr : u_field}))) return rc;
  pa_velocity vi;
  if (vel && (rc = check_velocity(c, vel, &vi, kind, src, who, {phi, phi0, out}))) return rc;
  const void* nuf;
  if ((rc = check_diffusivity(c, dif, &nuf, kind, who, {phi, phi0, out}, field_bytes(c)))) return rc;
  return step_any(c, phi, out, vel ? StepAdv{kind, 0.0, nullptr, &vi, -1} : StepAdv{kind, u, u_field, nullptr, -1}, 0.0, dt, phi0, c0, c1,
                  src, nuf);
}

int pa_march_nu(pa_ctx* c, void* phi, void* w1, void* w2, int order, int kind, double u, const void* u_field, const pa_velocity* vel,
                int self, double nu, double dt, int64_t nsteps, int* final, const pa_source* src, const pa_diffusivity* dif) {
  if (!dif || !dif->has) {   // the sibling itself
    if (vel) return pa_rk_march_vel(c, phi, w1, w2, order, kind, vel, nu, dt, nsteps, final, src);
    if (self) return pa_rk_march_self_src(c, phi, w1, w2, order, kind, nu, dt, nsteps, final, src);
    if (order == 1 && !w2) {
      const int rc = pa_euler_march_src(c, phi, w1, kind, u, u_field, nu, dt, nsteps, src);
      if (!rc && final) *final = (int)(nsteps & 1);
      return rc;
    }
    return pa_rk_march_src(c, phi, w1, w2, order, kind, u, u_field, nu, dt, nsteps, final, src);
  }
  const char* who = "pa_march_nu";
  int rc = check_march_call(c, who, order, kind, phi, w1, &w2, nsteps, final,
                            "distinct buffers (two for order 1, else three), a place for the result index and nsteps >= 0 are needed", 0);
  if (rc) return rc;
  const bool one = !vel && !self;
  if ((rc = check_source(c, &src, who, {phi, w1, w2, one ? u_field : nullptr}))) return rc;
  pa_velocity vi;
  if (vel && (rc = check_velocity(c, vel, &vi, kind, src, who, {phi, w1, w2}))) return rc;
  const void* nuf;
  if ((rc = check_diffusivity(c, dif, &nuf, kind, who, {phi, w1, w2}, field_bytes(c)))) return rc;
  if (one && overlaps(u_field, field_bytes(c), {phi, w1, w2}, field_bytes(c))) {
    pa_set_err(c, "%s: a frozen speed field must not be one of the march's buffers (self != 0 is the field that advects itself)", who);
    return PA_E_ARG;
  }
  PaRange range_("pyapes march with a diffusivity field");
  PA_HIP(c, hipSetDevice(c->device));
  void* const b[3] = {phi, w1, w2};
  return PA_BY_DTYPE(c, march_nu_t, c, b, order, kind, one ? u : 0.0, one ? u_field : nullptr, !vel && self != 0, vel ? &vi : nullptr, dt,
                     nsteps, final, src, nuf);
}

int pa_euler_step_src(pa_ctx* c, const void* in, void* out, int kind, double u, const void* u_field, double nu, double dt,
                      const pa_source* src) {
  if (!c || !c->grid_set) return PA_E_STATE;
  int rc = pa_check_div_kind(c, kind, "pa_euler_step");
  if (rc) return rc;
  if (in == out) { pa_set_err(c, "pa_euler_step: in-place step is not allowed"); return PA_E_ARG; }
  if ((rc = check_source(c, &src, "pa_euler_step_src", {in, out, u_field}))) return rc;
  return step_any(c, in, out, StepAdv{kind, u, u_field, nullptr, -1}, nu, dt, nullptr, 0.0, 0.0, src);
}

int pa_euler_step(pa_ctx* c, const void* in, void* out, int kind, double u, const void* u_field, double nu,
                  double dt) {
  return pa_euler_step_src(c, in, out, kind, u, u_field, nu, dt, nullptr);
}

int pa_euler_march_src(pa_ctx* c, void* phi, void* tmp, int kind, double u, const void* u_field, double nu, double dt,
                       int64_t nsteps, const pa_source* src) {
  int final = 0;
  void* w2 = nullptr;
  int rc = check_march_call(c, "pa_euler_march", 1, kind, phi, tmp, &w2, nsteps, &final, "bad buffers / step count", 0);
  if (rc) return rc;
  if ((rc = check_source(c, &src, "pa_euler_march_src", {phi, tmp, u_field}))) return rc;
  PaRange range_("pyapes explicit Euler march");
  PA_HIP(c, hipSetDevice(c->device));
  void* const b[3] = {phi, tmp, nullptr};
  return PA_BY_DTYPE(c, march_one_t, c, b, 1, kind, u, u_field, false, nu, dt, nsteps, &final, src);
}

int pa_euler_march(pa_ctx* c, void* phi, void* tmp, int kind, double u, const void* u_field, double nu, double dt,
                   int64_t nsteps) {
  return pa_euler_march_src(c, phi, tmp, kind, u, u_field, nu, dt, nsteps, nullptr);
}

int pa_rk_stage_src(pa_ctx* c, const void* phi, const void* phi0, void* out, double c0, double c1, int kind, double u,
                    const void* u_field, double nu, double dt, const pa_source* src) {
  if (!c || !c->grid_set) return PA_E_STATE;
  int rc = pa_check_div_kind(c, kind, "pa_rk_stage");
  if (rc) return rc;
  if (!phi || !phi0 || !out || out == phi || out == phi0) {
    pa_set_err(c, "pa_rk_stage: out must be a buffer of its own (not phi, not phi0)");
    return PA_E_ARG;
  }
  if (on_slab(c)) { pa_set_err(c, "pa_rk_stage: single GPU only (no slab stages)"); return PA_E_STATE; }
  if ((rc = check_source(c, &src, "pa_rk_stage_src", {phi, phi0, out, u_field}))) return rc;
  return step_any(c, phi, out, StepAdv{kind, u, u_field, nullptr, -1}, nu, dt, phi0, c0, c1, src);
}

int pa_rk_stage(pa_ctx* c, const void* phi, const void* phi0, void* out, double c0, double c1, int kind, double u,
                const void* u_field, double nu, double dt) {
  return pa_rk_stage_src(c, phi, phi0, out, c0, c1, kind, u, u_field, nu, dt, nullptr);
}

int pa_rk_march_src(pa_ctx* c, void* phi, void* w1, void* w2, int order, int kind, double u, const void* u_field, double nu,
                    double dt, int64_t nsteps, int* final, const pa_source* src) {
  int rc = check_march_call(c, "pa_rk_march", order, kind, phi, w1, &w2, nsteps, final,
                            "three distinct buffers, a place for the result index and nsteps >= 0 are needed", MC_W2_ALWAYS | MC_NO_SLAB);
  if (rc) return rc;
  if ((rc = check_source(c, &src, "pa_rk_march_src", {phi, w1, w2, u_field}))) return rc;
  PaRange range_(order == 1 ? "pyapes explicit Euler march" : "pyapes SSP Runge-Kutta march");
  PA_HIP(c, hipSetDevice(c->device));
  void* const b[3] = {phi, w1, w2};
  return PA_BY_DTYPE(c, march_one_t, c, b, order, kind, u, u_field, false, nu, dt, nsteps, final, src);
}

int pa_rk_march(pa_ctx* c, void* phi, void* w1, void* w2, int order, int kind, double u, const void* u_field, double nu,
                double dt, int64_t nsteps, int* final) {
  return pa_rk_march_src(c, phi, w1, w2, order, kind, u, u_field, nu, dt, nsteps, final, nullptr);
}

int pa_rk_march_self_src(pa_ctx* c, void* phi, void* w1, void* w2, int order, int kind, double nu, double dt, int64_t nsteps,
                         int* final, const pa_source* src) {
  int rc = check_march_call(c, "pa_rk_march_self", order, kind, phi, w1, &w2, nsteps, final,
                            "distinct buffers (two for order 1, else three), a place for the result index and nsteps >= 0 are needed", MC_NO_SLAB);
  if (rc) return rc;
  if ((rc = check_source(c, &src, "pa_rk_march_self_src", {phi, w1, w2}))) return rc;
  PaRange range_(order == 1 ? "pyapes explicit Euler march" : "pyapes SSP Runge-Kutta march, self-advected");
  PA_HIP(c, hipSetDevice(c->device));
  void* const b[3] = {phi, w1, w2};
  return PA_BY_DTYPE(c, march_one_t, c, b, order, kind, 0.0, nullptr, true, nu, dt, nsteps, final, src);
}

int pa_rk_march_self(pa_ctx* c, void* phi, void* w1, void* w2, int order, int kind, double nu, double dt, int64_t nsteps,
                     int* final) {
  return pa_rk_march_self_src(c, phi, w1, w2, order, kind, nu, dt, nsteps, final, nullptr);
}

}  // extern "C"
