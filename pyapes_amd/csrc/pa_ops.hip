// pa_ops.hip -- generic (any dimension / extent / term list) operator kernels and the explicit entry
// points: y = A x, Laplacian / Grad / Div with edge=True post-passes, rhs adjustment of Solver.set_eq,
// explicit Euler step.  The tiled kernels (pa_cg3d*.hip) take over where they apply.
#include "pa_host.h"

#include <math.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <new>

// ---- y = A(x) (pyapes/solver/ops.py:122-154) -----------------------------------------
template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_aop(DevGeom G, DevEq<T> E, Vec<T> xv, T* __restrict__ y,
                                                   int interior_only) {
  FieldAcc<T> acc{xv};
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < G.ncell;
       idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t i, j, k;
    pa_decode(G, idx, i, j, k);
    T out = (T)0;
    if (!interior_only || pa_in_S(G, i, j, k)) {
      T xc = xv.p[idx];
      out = pa_apply_terms<T>(G, E, acc, i, j, k, xc);
    }
    y[idx] = out;
  }
}

// ---- explicit gradient: y[(a), n...] (fdc.py:80-87) -----------------------------------
template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_grad(DevGeom G, DevEq<T> E, Vec<T> xv, T* __restrict__ y,
                                                    int nd) {
  FieldAcc<T> acc{xv};
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < G.ncell;
       idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t i, j, k;
    pa_decode(G, idx, i, j, k);
    int64_t g[3], N[3];
    pa_gidx(G, i, j, k, g, N);
    T xc = xv.p[idx];
    for (int a = 3 - nd; a < 3; ++a) {
      T cP = E.grd.g[a], cC = (T)0, cM = E.grd.mg[a];
      int rc = pa_row_case(G, a, g[a], N[a], G.treat);
      if (rc == 1) { cP = E.grd.lo_p[a]; cC = E.grd.lo_c[a]; cM = (T)0; }
      if (rc == 2) { cP = (T)0; cC = E.grd.hi_c[a]; cM = E.grd.hi_m[a]; }
      if (G.bct[2 * a] == 4 && g[a] == 1) cM = (T)0;
      if (G.bct[2 * a + 1] == 4 && g[a] == N[a] - 2) cP = (T)0;
      T xp, xm;
      pa_nbrs<T>(G, acc, a, i, j, k, xp, xm);
      T s = cP * xp;
      T m = cC * xc;
      s = s + m;
      m = cM * xm;
      s = s + m;
      y[(int64_t)(a - (3 - nd)) * G.ncell + idx] = s;
    }
  }
}

// ---- edge=True one-sided boundary formulas (fdc.py:203-288) ---------------------------
// mode 0: laplacian (y is one field; the LAST mesh axis whose index is on the boundary wins,
// because the reference overwrites faces axis by axis); mode 1: grad (y[a] on faces normal to a).
template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_edge(DevGeom G, DevEq<T> E, const T* __restrict__ x,
                                                    T* __restrict__ y, int nd, int mode, T u = (T)0,
                                                    const T* __restrict__ u_f = nullptr) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < G.ncell;
       idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t i, j, k;
    pa_decode(G, idx, i, j, k);
    int64_t c[3] = {i, j, k};
    int64_t n[3] = {G.n0, G.n1, G.n2};
    int64_t st[3] = {G.s0, G.s1, 1};
    if (mode == 0) {
      int sel = -1;
      for (int a = 3 - nd; a < 3; ++a)
        if (c[a] == 0 || c[a] == n[a] - 1) sel = a;
      if (sel < 0) continue;
      int64_t dir = (c[sel] == 0) ? 1 : -1;
      T v0 = x[idx], v1 = x[idx + dir * st[sel]], v2 = x[idx + 2 * dir * st[sel]],
        v3 = x[idx + 3 * dir * st[sel]];
      T s = (T)2 * v0;
      T m = (T)5 * v1;
      s = s - m;
      m = (T)4 * v2;
      s = s + m;
      s = s - v3;
      T h2 = E.grd.h[sel] * E.grd.h[sel];
      y[idx] = s / h2;
    } else if (mode == 1) {
      for (int a = 3 - nd; a < 3; ++a) {
        if (!(c[a] == 0 || c[a] == n[a] - 1)) continue;
        int64_t dir = (c[a] == 0) ? 1 : -1;
        T v0 = x[idx], v1 = x[idx + dir * st[a]], v2 = x[idx + 2 * dir * st[a]];
        T s = (T)1.5 * v0;
        T m = (T)2 * v1;
        s = s - m;
        m = (T)0.5 * v2;
        s = s + m;
        if (c[a] == 0) s = -s;
        y[(int64_t)(a - (3 - nd)) * G.ncell + idx] = s / E.grd.h[a];
      }
    } else {
      // Div, 1-D (fdc.py:316-348): -+(3/2 v0 - 2 v1 + 1/2 v2) / dx * adv on the two end nodes
      const int a = 2;
      if (!(c[a] == 0 || c[a] == n[a] - 1)) continue;
      int64_t dir = (c[a] == 0) ? 1 : -1;
      T v0 = x[idx], v1 = x[idx + dir], v2 = x[idx + 2 * dir];
      T s = (T)1.5 * v0;
      T m = (T)2 * v1;
      s = s - m;
      m = (T)0.5 * v2;
      s = s + m;
      if (c[a] == 0) s = -s;
      s = s / E.grd.h[a];
      y[idx] = s * (u_f ? u_f[idx] : u);
    }
  }
}

// ---- rhs adjustment of Solver.set_eq (ops.py:63-77; fdc.py:426-458, 505-540, 667-694) --
template <typename T>
struct RhsFace {
  int type;       // PA_BC_*
  T sval;         // scalar V
  const T* vals;  // per-node V or null
};
template <typename T>
struct RhsArgs {
  RhsFace<T> f[6];
  int order[6];   // internal face ids in list order
  int nfaces;
  T c23, c13;     // (T)(2/3), (T)(1/3)
  T h[3];
  // only nodes one step inside a Neumann face are touched: the kernel visits those layers, not the mesh
  int nlay;             // number of layers (<= 6); 0: visit every cell
  int lay_axis[6];      // internal axis of layer w
  int64_t lay_pos[6];   // its LOCAL index along that axis
  int64_t lay_start[7]; // prefix sums of the layer sizes
};

template <typename T>
__device__ __forceinline__ T pa_face_val(const DevGeom& G, const RhsFace<T>& F, int a, int64_t i, int64_t j,
                                         int64_t k) {
  if (!F.vals) return F.sval;
  if (a == 0) return F.vals[j * G.n2 + k];
  if (a == 1) return F.vals[i * G.n2 + k];
  return F.vals[i * G.n1 + j];
}

template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_rhs_adjust(DevGeom G, DevEq<T> E, RhsArgs<T> R,
                                                          T* __restrict__ rhs) {
  const int64_t total = R.nlay ? R.lay_start[R.nlay] : G.ncell;
  for (int64_t tix = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; tix < total;
       tix += (int64_t)gridDim.x * blockDim.x) {
    int64_t idx = tix, i, j, k;
    if (R.nlay) {
      // which layer, which node of it; a node on two layers belongs to the first one
      int wsel = 0, ax = 0;
      int64_t q = 0, pos = 0;
#pragma unroll
      for (int w = 0; w < 6; ++w)
        if (w < R.nlay && tix >= R.lay_start[w] && tix < R.lay_start[w + 1]) {
          wsel = w; ax = R.lay_axis[w]; pos = R.lay_pos[w]; q = tix - R.lay_start[w];
        }
      if (ax == 0) { i = pos; j = q / G.n2; k = q - j * G.n2; }
      else if (ax == 1) { j = pos; i = q / G.n2; k = q - i * G.n2; }
      else { k = pos; i = q / G.n1; j = q - i * G.n1; }
      bool dup = false;
#pragma unroll
      for (int w = 0; w < 6; ++w)
        if (w < wsel) {
          const int64_t cw = R.lay_axis[w] == 0 ? i : (R.lay_axis[w] == 1 ? j : k);
          if (cw == R.lay_pos[w]) dup = true;
        }
      if (dup) continue;
      idx = i * G.s0 + j * G.s1 + k;
    } else {
      pa_decode(G, idx, i, j, k);
    }
    int64_t g[3], N[3];
    pa_gidx(G, i, j, k, g, N);
    T val = rhs[idx];
    bool touched = false;
    for (int q = 0; q < E.nterms; ++q) {
      const DevTerm<T>& t = E.t[q];
      T adj = (T)0;
      bool any = false;
      // reference loop nest: for axis j: for bc in list order (only faces normal to j contribute)
      for (int a = 0; a < 3; ++a) {
        if (!G.act[a]) continue;
        for (int w = 0; w < R.nfaces; ++w) {
          int fc = R.order[w];
          if ((fc >> 1) != a) continue;
          if (R.f[fc].type != 2) continue;
          int side = fc & 1;
          int64_t prev = side == 0 ? pa_wrap(1, N[a]) : pa_wrap(N[a] - 2, N[a]);
          if (g[a] != prev) continue;
          T V = pa_face_val<T>(G, R.f[fc], a, i, j, k);
          T nv = side == 0 ? (T)-1 : (T)1;
          T vn = V * nv;
          if (t.kind == 0) {            // laplacian: += (2/3 - alpha)(V n)/h   (fdc.py:440-453)
            T f23 = (E.rz && a == PA_RZ_AXIS) ? E.rz[3 * E.rz_n + g[a]] : R.c23;
            T s = f23 * vn;
            s = s / R.h[a];
            adj = adj + s;
          } else if (t.kind == 1) {     // grad: -= (1/3)(V n) * 1      (fdc.py:526-537)
            T s = R.c13 * vn;
            adj = adj - s;
          } else {                      // div: -= (1/3)(V n) * gamma   (fdc.py:680-686)
            T ucen = t.u_f ? t.u_f[idx] : t.u;
            T gm;
            if (t.kind == 2) gm = (T)2 * ucen;
            else {
              // upwind: lower face uses 2*max(u,0), upper face 2*min(u,0)
              T mx = ucen > (T)0 ? ucen : (T)0, mn = ucen < (T)0 ? ucen : (T)0;
              gm = side == 0 ? (T)2 * mx : (T)2 * mn;
            }
            T s = R.c13 * vn;
            s = s * gm;
            adj = adj - s;
          }
          any = true;
        }
      }
      if (any) { val = val + adj; touched = true; }
    }
    if (touched) rhs[idx] = val;
  }
}


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

// adv = (+0) + t_0 + t_1 + t_2 over the active axes: the per-axis term of pa_apply_terms' scheme `kind` (central, QUICK,
// upwind), operation for operation, with axis a's own speed W.f[a] / W.val[a] in the place of the one speed
template <typename T>
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
      T cP = up, cC = (T)0 * ucen, cM = -um;
      if (G.bct[2 * a] == 4 && g[a] == 1) cM = (T)0;
      if (G.bct[2 * a + 1] == 4 && g[a] == N[a] - 2) cP = (T)0;
      cP = cP / grd.h2[a];
      cC = cC / grd.h2[a];
      cM = cM / grd.h2[a];
      T s = cP * xp;
      T m = cC * xc;
      s = s + m;
      m = cM * xm;
      s = s + m;
      ax = ax + s;
    } else {
      const T upl = ucen > (T)0 ? ucen : (T)0;
      const T umi = ucen < (T)0 ? ucen : (T)0;
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

template <typename T, bool STG = false, bool SRC = false, bool VEL = false>
__global__ void __launch_bounds__(PA_BLOCK) k_euler(DevGeom G, DevEq<T> Elap, DevEq<T> Eadv, Vec<T> pv,
                                                     T* __restrict__ out, T nu, T dt, EulerStage<T, STG> S = {},
                                                     EulerSrc<T, SRC> Q = {}, EulerVel<T, VEL> W = {}) {
  FieldAcc<T> acc{pv};
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < G.ncell;
       idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t i, j, k;
    pa_decode(G, idx, i, j, k);
    T pc = pv.p[idx];
    T v = pc;
    if (pa_in_S(G, i, j, k)) {
      T lap = pa_apply_terms<T>(G, Elap, acc, i, j, k, pc);
      T adv;
      if constexpr (VEL) adv = pa_adv_vel<T>(G, Elap.grd, W, acc, i, j, k, pc);
      else adv = pa_apply_terms<T>(G, Eadv, acc, i, j, k, pc);
      T a = nu * lap;
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

// the stage where it cannot be fused (a periodic face, euler_t): x <- c0 * phi0 + c1 * x, x the finished Euler step
template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_rk_combine(T* __restrict__ x, const T* __restrict__ phi0, T c0, T c1, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    T t0 = c0 * phi0[i];
    T t1 = c1 * x[i];
    x[i] = t0 + t1;
  }
}

// ---- host side ----------------------------------------------------------------------------------
// Grad inside an operator sum only makes sense in 1-D (the reference reshapes the
// (1, mesh.dim, n...) result onto the target, ops.py:145-147)
int pa_check_eq_applicable(pa_ctx* c) {
  for (int q = 0; q < c->nterms; ++q)
    if (c->terms[q].kind == PA_OP_GRAD && c->ndim != 1) {
      pa_set_err(c, "Grad in a solver equation is 1-D only (ops.py:145-147 view)");
      return PA_E_ARG;
    }
  return PA_OK;
}

// -------- typed implementations behind the remaining entry points ------------------------
template <typename T>
static int aop_t(pa_ctx* c, const T* x, T* y, int interior_only, int nterms, const pa_term* terms) {
  DevEq<T> E;
  pa_build_eq<T>(c, nterms, terms, E);
  Vec<T> xv = pa_vec_self<T>(c, x);
  if (c->G.n0 != c->G.g0 && c->ndim == 3) {
    // slab: ghost planes of x must have been supplied
    if (!c->x_glo || !c->x_ghi) { pa_set_err(c, "pa_aop on a slab needs ghost planes (pa_x_ghost_set)"); return PA_E_STATE; }
    xv.glo = (const T*)c->x_glo;
    xv.ghi = (const T*)c->x_ghi;
  }
  int fr = pa_tile3d_aop<T>(c, E, xv, y, interior_only);
  if (fr < 0) return fr;
  if (fr == 0)
    hipLaunchKernelGGL(k_aop<T>, dim3(pa_grid_blocks(c->G.ncell)), dim3(PA_BLOCK), 0, c->stream, c->G, E, xv, y,
                       interior_only);
  PA_HIP(c, hipGetLastError());
  return PA_OK;
}

template <typename T>
static int rhs_adjust_t(pa_ctx* c, T* rhs) {
  DevEq<T> E;
  pa_build_eq<T>(c, c->nterms, c->terms, E);
  RhsArgs<T> R;
  memset(&R, 0, sizeof(R));
  bool any = false;
  for (int f = 0; f < 6; ++f) {
    R.f[f].type = c->bc[f].type;
    R.f[f].sval = (T)c->bc[f].value;
    R.f[f].vals = (const T*)c->bc[f].vals;
    if (c->bc[f].type == PA_BC_NEUMANN) any = true;
  }
  R.nfaces = c->nbc;
  for (int w = 0; w < c->nbc; ++w) R.order[w] = c->bc_order[w];
  R.c23 = (T)(2.0 / 3.0);
  R.c13 = (T)(1.0 / 3.0);
  for (int a = 0; a < 3; ++a) R.h[a] = (T)c->dx[a];
  if (!any) return PA_OK;
  // the layers one step inside each Neumann face (global node 1 / N-2 of its axis), as far as this rank owns them
  const DevGeom& G = c->G;
  const int64_t Ng[3] = {G.g0, G.n1, G.n2}, nl[3] = {G.n0, G.n1, G.n2};
  R.nlay = 0;
  R.lay_start[0] = 0;
  for (int f = 0; f < 6; ++f) {
    const int a = f >> 1;
    if (c->bc[f].type != PA_BC_NEUMANN || !G.act[a]) continue;
    int64_t prev = (f & 1) == 0 ? 1 : Ng[a] - 2;
    prev = ((prev % Ng[a]) + Ng[a]) % Ng[a];
    const int64_t pos = a == 0 ? prev - G.off0 : prev;
    if (pos < 0 || pos >= nl[a]) continue;   // another rank's plane
    const int64_t size = a == 0 ? G.n1 * G.n2 : (a == 1 ? G.n0 * G.n2 : G.n0 * G.n1);
    R.lay_axis[R.nlay] = a;
    R.lay_pos[R.nlay] = pos;
    R.lay_start[R.nlay + 1] = R.lay_start[R.nlay] + size;
    ++R.nlay;
  }
  if (R.nlay == 0) return PA_OK;             // no Neumann layer on this rank
  if (c->rhs_full) R.nlay = 0;   // option "rhs_full" (tests: same bits)
  const int64_t work = R.nlay ? R.lay_start[R.nlay] : G.ncell;
  hipLaunchKernelGGL(k_rhs_adjust<T>, dim3(pa_grid_blocks(work)), dim3(PA_BLOCK), 0, c->stream, c->G, E, R, rhs);
  PA_HIP(c, hipGetLastError());
  return PA_OK;
}

template <typename T>
static int lap_t(pa_ctx* c, const T* x, T* y, int edge) {
  pa_term t;
  memset(&t, 0, sizeof(t));
  t.kind = PA_OP_LAPLACIAN; t.sign = 1.0; t.has_coeff = 0;
  int rc = aop_t<T>(c, x, y, 0, 1, &t);
  if (rc) return rc;
  if (edge) {
    for (int a = 0; a < c->ndim; ++a) {
      int64_t n = a + (3 - c->ndim) == 0 ? c->G.n0 : (a + (3 - c->ndim) == 1 ? c->G.n1 : c->G.n2);
      if (n < 4) { pa_set_err(c, "edge laplacian needs >= 4 nodes per axis"); return PA_E_ARG; }
    }
    if (c->G.n0 != c->G.g0 && c->ndim == 3) { pa_set_err(c, "edge operators are single-GPU only"); return PA_E_ARG; }
    DevEq<T> E;
    pa_build_eq<T>(c, 1, &t, E);
    hipLaunchKernelGGL(k_edge<T>, dim3(pa_grid_blocks(c->G.ncell)), dim3(PA_BLOCK), 0, c->stream, c->G, E, x, y,
                       c->ndim, 0);
    PA_HIP(c, hipGetLastError());
  }
  return PA_OK;
}

template <typename T>
static int grad_t(pa_ctx* c, const T* x, T* y, int edge) {
  pa_term t;
  memset(&t, 0, sizeof(t));
  t.kind = PA_OP_GRAD; t.sign = 1.0;
  DevEq<T> E;
  pa_build_eq<T>(c, 1, &t, E);
  Vec<T> xv = pa_vec_self<T>(c, x);
  if (c->G.n0 != c->G.g0 && c->ndim == 3) {
    if (!c->x_glo || !c->x_ghi) { pa_set_err(c, "pa_grad on a slab needs ghost planes"); return PA_E_STATE; }
    xv.glo = (const T*)c->x_glo; xv.ghi = (const T*)c->x_ghi;
  }
  int fr = pa_tile3d_grad<T>(c, xv, y, c->ndim);
  if (fr < 0) return fr;
  if (fr == 0)
    hipLaunchKernelGGL(k_grad<T>, dim3(pa_grid_blocks(c->G.ncell)), dim3(PA_BLOCK), 0, c->stream, c->G, E, xv, y,
                       c->ndim);
  if (edge) {
    if (c->G.n0 != c->G.g0 && c->ndim == 3) { pa_set_err(c, "edge operators are single-GPU only"); return PA_E_ARG; }
    hipLaunchKernelGGL(k_edge<T>, dim3(pa_grid_blocks(c->G.ncell)), dim3(PA_BLOCK), 0, c->stream, c->G, E, x, y,
                       c->ndim, 1);
  }
  PA_HIP(c, hipGetLastError());
  return PA_OK;
}

// `who`: the entry point, for the messages of the QUICK checks
static int check_div_kind(pa_ctx* c, int kind, const char* who = "pa_div") {
  if (kind == PA_OP_DIV_QUICK) {
    // the reach of 2: no ghost planes at that distance, no r-dependent rows.  Neumann / symmetry faces are allowed -- the
    // fallback next to a face reads BC-filled values only
    if (c->slab || (c->G.n0 != c->G.g0 && c->ndim == 3)) { pa_set_err(c, "%s: Div quick is single GPU only (no slabs)", who); return PA_E_STATE; }
    if (c->coord != PA_COORD_XYZ) { pa_set_err(c, "%s: Div quick is for xyz meshes (no axisymmetric rows)", who); return PA_E_ARG; }
    const int64_t n[3] = {c->G.n0, c->G.n1, c->G.n2};
    for (int a = 0; a < 3; ++a)
      if (c->G.act[a] && n[a] < 5) { pa_set_err(c, "%s: Div quick needs at least 5 nodes per axis (%lld)", who, (long long)n[a]); return PA_E_ARG; }
    return PA_OK;
  }
  if (kind != PA_OP_DIV_CENTRAL && kind != PA_OP_DIV_UPWIND_COMPAT && kind != PA_OP_DIV_UPWIND) {
    pa_set_err(c, "bad div kind %d", kind);
    return PA_E_ARG;
  }
  if (kind == PA_OP_DIV_CENTRAL)
    for (int f = 0; f < 6; ++f)
      if (c->G.treat[f]) {
        pa_set_err(c, "central Div with neumann/symmetry faces: the reference raises IndexError (fdc.py:583)");
        return PA_E_ARG;
      }
  return PA_OK;
}

// phi0 != null: the Runge-Kutta stage out = B( c0 phi0 + c1 E(in) ) (pa_rk_stage), on the path the Euler step takes
template <typename T>
static int euler_t(pa_ctx* c, const T* in, T* out, int kind, double u, const void* u_field, double nu, double dt,
                   const T* phi0 = nullptr, double c0 = 0.0, double c1 = 0.0, const pa_source* src = nullptr) {
  if (phi0) {
    // A stage combines the Euler STEP, BC fill included.  For dirichlet / neumann / symmetry faces the fill rewrites its
    // nodes from interior-set values alone, so filling once, after the combination, gives the same bits and the stage is
    // one kernel.  The periodic fill is not of that kind: its lower face reads the upper face's value BEFORE the fill
    // rewrites it (bcs.py:253-262: x[0] = x[1] - x[n-1] + x[n-2]), and those nodes belong to the interior set -- B(c0 phi0 +
    // c1 e) would see the raw stencil value there where the Euler step hands on its filled one.  With a periodic face the
    // stage is therefore the step itself, then the combination in place, then the fill.
    bool periodic = false;
    for (int f = 0; f < 6; ++f) periodic = periodic || (c->G.act[f >> 1] && c->bc[f].type == PA_BC_PERIODIC);
    if (periodic) {
      if (int rc = euler_t<T>(c, in, out, kind, u, u_field, nu, dt, nullptr, 0.0, 0.0, src)) return rc;   // the source enters in the step only
      static int dbg = -1;
      if (dbg < 0) dbg = getenv("PYAPES_HIP_DEBUG") ? 8 : 0;
      if (dbg > 0) { --dbg; fprintf(stderr, "[pyapes_hip] k_rk_combine (RK stage, periodic face): Euler step, then %lld cells in place\n", (long long)c->G.ncell); }
      if (c->profile) (void)hipEventRecord(c->pev[0], c->stream);
      hipLaunchKernelGGL(k_rk_combine<T>, dim3(pa_grid_blocks(c->G.ncell)), dim3(PA_BLOCK), 0, c->stream, out, phi0, (T)c0,
                         (T)c1, c->G.ncell);
      if (c->profile) pa_profile_stop(c, 0);
      PA_HIP(c, hipGetLastError());
      return pa_bc_apply_auto<T>(c, out, false);
    }
  }
  pa_term tl, ta;
  memset(&tl, 0, sizeof(tl));
  memset(&ta, 0, sizeof(ta));
  tl.kind = PA_OP_LAPLACIAN; tl.sign = 1.0;
  ta.kind = kind; ta.sign = 1.0; ta.u = u; ta.u_field = u_field;
  DevEq<T> El, Ea;
  pa_build_eq<T>(c, 1, &tl, El);
  pa_build_eq<T>(c, 1, &ta, Ea);
  Vec<T> pv = pa_vec_self<T>(c, in);
  if (c->G.n0 != c->G.g0 && c->ndim == 3) {
    // a slab (pyapes_amd/slab.py SlabEuler): ghost planes from pa_slab_set; a NULL one marks a physical end, whose
    // boundary plane no interior node reads across -- the field's own end plane stands in for the speculative loads
    if (!c->slab) { pa_set_err(c, "pa_euler_step on a slab needs pa_slab_set (ghost planes)"); return PA_E_STATE; }
    pv.glo = c->x_glo ? (const T*)c->x_glo : in;
    pv.ghi = c->x_ghi ? (const T*)c->x_ghi : in + (c->G.n0 - 1) * c->G.s0;
  }
  if (c->profile) (void)hipEventRecord(c->pev[0], c->stream);   // slot 0: the step kernel (without its BC fill)
  // QUICK: k_sfq or the generic kernel (the tiled paths of pa_tile3d_euler do not know the kind and decline it)
  // a source: the SRC instantiations of k_sf / k_sfq or the generic kernel (k_cg3d's Euler phase takes none)
  int fr = kind == PA_OP_DIV_QUICK ? pa_sfq_euler<T>(c, pv, out, u, u_field, nu, dt, phi0, c0, c1, src)
                                   : pa_tile3d_euler<T>(c, pv, out, kind, u, u_field, nu, dt, 0, phi0, c0, c1, src);
  if (fr < 0) return fr;
  if (fr == 0 && src) {
    static int dbg = -1;   // (one budget for every mesh and both forms: larger than an instantiation's 8)
    if (dbg < 0) dbg = getenv("PYAPES_HIP_DEBUG") ? 64 : 0;
    if (dbg > 0) { --dbg; fprintf(stderr, "[pyapes_hip] k_euler%s (source): generic kernel, %lld cells\n", phi0 ? " (RK stage)" : "", (long long)c->G.ncell); }
    const EulerSrc<T, true> Q{(const T*)src->field, (T)src->value};
    if (phi0)
      hipLaunchKernelGGL((k_euler<T, true, true>), dim3(pa_grid_blocks(c->G.ncell)), dim3(PA_BLOCK), 0, c->stream, c->G, El, Ea,
                         pv, out, (T)nu, (T)dt, EulerStage<T, true>{phi0, (T)c0, (T)c1}, Q);
    else
      hipLaunchKernelGGL((k_euler<T, false, true>), dim3(pa_grid_blocks(c->G.ncell)), dim3(PA_BLOCK), 0, c->stream, c->G, El, Ea,
                         pv, out, (T)nu, (T)dt, EulerStage<T, false>{}, Q);
  } else if (fr == 0 && phi0) {
    static int dbg = -1;
    if (dbg < 0) dbg = getenv("PYAPES_HIP_DEBUG") ? 8 : 0;
    if (dbg > 0) { --dbg; fprintf(stderr, "[pyapes_hip] k_euler (RK stage): generic kernel, %lld cells\n", (long long)c->G.ncell); }
    hipLaunchKernelGGL((k_euler<T, true>), dim3(pa_grid_blocks(c->G.ncell)), dim3(PA_BLOCK), 0, c->stream, c->G, El, Ea, pv,
                       out, (T)nu, (T)dt, EulerStage<T, true>{phi0, (T)c0, (T)c1});
  } else if (fr == 0)
    hipLaunchKernelGGL(k_euler<T>, dim3(pa_grid_blocks(c->G.ncell)), dim3(PA_BLOCK), 0, c->stream, c->G, El, Ea, pv,
                       out, (T)nu, (T)dt);
  if (c->profile) pa_profile_stop(c, 0);
  PA_HIP(c, hipGetLastError());
  // slab mode: the step kernel alone.  The fill of a periodic axis 0 reads planes of the NEW field that live on the
  // other end rank of the ring, so the driver exchanges those first and then calls pa_apply_bc itself.
  if (c->slab) return PA_OK;
  return pa_bc_apply_auto<T>(c, out, false);
}

// One step of the march in the "BC on load" form (pa_sf_kernel.h): the step kernel alone, no fill behind it -- the
// boundary nodes of `out` stay whatever they were.  1: launched; 0: the form does not apply here; < 0: error.
template <typename T>
static int euler_bcl_t(pa_ctx* c, const T* in, T* out, int kind, double u, const void* u_field, double nu, double dt,
                       const T* phi0 = nullptr, double c0 = 0.0, double c1 = 0.0, const pa_source* src = nullptr) {
  Vec<T> pv = pa_vec_self<T>(c, in);
  if (c->profile) (void)hipEventRecord(c->pev[0], c->stream);
  const int fr = pa_tile3d_euler<T>(c, pv, out, kind, u, u_field, nu, dt, 1, phi0, c0, c1, src);
  if (fr <= 0) return fr;
  if (c->profile) pa_profile_stop(c, 0);
  return 1;
}

// The Euler step (phi0 null) or the fused stage with a velocity (pa_*_vel), vel indexed by INTERNAL axis: k_sf's VEL
// instantiations where pa_tile3d_euler_vel takes the launch, else the generic k_euler<..., VEL>; then the ordered BC fill.
// A periodic face: the step, k_rk_combine in place, the fill -- as euler_t and for its reason.
// own >= 0 (momentum_march_t): vel->field[own] is `in` itself -- the target is a component of the velocity.  Nothing on the way
// needs the speed fields to be distinct from the field read through the stencil: cg3d_mode ORs the pointers for their alignment,
// sf_applies does not look at them, and the kernels read every operand through plain (non-restrict) global loads; `out` alone is
// written, and it is a buffer of its own.
template <typename T>
static int euler_vel_t(pa_ctx* c, const T* in, T* out, int kind, const pa_velocity* vel, double nu, double dt,
                       const T* phi0, double c0, double c1, const pa_source* src, int own = -1) {
  if (phi0) {
    bool periodic = false;
    for (int f = 0; f < 6; ++f) periodic = periodic || (c->G.act[f >> 1] && c->bc[f].type == PA_BC_PERIODIC);
    if (periodic) {
      if (int rc = euler_vel_t<T>(c, in, out, kind, vel, nu, dt, nullptr, 0.0, 0.0, src, own)) return rc;
      if (c->profile) (void)hipEventRecord(c->pev[0], c->stream);
      hipLaunchKernelGGL(k_rk_combine<T>, dim3(pa_grid_blocks(c->G.ncell)), dim3(PA_BLOCK), 0, c->stream, out, phi0, (T)c0,
                         (T)c1, c->G.ncell);
      if (c->profile) pa_profile_stop(c, 0);
      PA_HIP(c, hipGetLastError());
      return pa_bc_apply_auto<T>(c, out, false);
    }
  }
  pa_term tl;
  memset(&tl, 0, sizeof(tl));
  tl.kind = PA_OP_LAPLACIAN; tl.sign = 1.0;
  DevEq<T> El;
  pa_build_eq<T>(c, 1, &tl, El);
  Vec<T> pv = pa_vec_self<T>(c, in);
  if (c->profile) (void)hipEventRecord(c->pev[0], c->stream);
  const int fr = pa_tile3d_euler_vel<T>(c, pv, out, kind, vel, nu, dt, phi0, c0, c1, src, own);
  if (fr < 0) {
    if (c->profile) pa_profile_stop(c, 0);
    return fr;
  }
  if (fr == 0) {
    static int dbg = -1;
    if (dbg < 0) dbg = getenv("PYAPES_HIP_DEBUG") ? 64 : 0;
    if (dbg > 0) { --dbg; fprintf(stderr, "[pyapes_hip] k_euler%s%s (velocity): generic kernel, %lld cells\n", phi0 ? " (RK stage)" : "", src ? " (source)" : "", (long long)c->G.ncell); }
    EulerVel<T, true> W;
    for (int a = 0; a < 3; ++a) { W.f[a] = (const T*)vel->field[a]; W.val[a] = (T)vel->value[a]; }
    W.kind = kind;
    const dim3 grid(pa_grid_blocks(c->G.ncell)), block(PA_BLOCK);   // (below, the second El stands in for Eadv: unread with VEL)
    const EulerStage<T, true> S{phi0, (T)c0, (T)c1};
    if (src) {
      const EulerSrc<T, true> Q{(const T*)src->field, (T)src->value};
      if (phi0) hipLaunchKernelGGL((k_euler<T, true, true, true>), grid, block, 0, c->stream, c->G, El, El, pv, out, (T)nu, (T)dt, S, Q, W);
      else hipLaunchKernelGGL((k_euler<T, false, true, true>), grid, block, 0, c->stream, c->G, El, El, pv, out, (T)nu, (T)dt, EulerStage<T, false>{}, Q, W);
    } else {
      if (phi0) hipLaunchKernelGGL((k_euler<T, true, false, true>), grid, block, 0, c->stream, c->G, El, El, pv, out, (T)nu, (T)dt, S, EulerSrc<T, false>{}, W);
      else hipLaunchKernelGGL((k_euler<T, false, false, true>), grid, block, 0, c->stream, c->G, El, El, pv, out, (T)nu, (T)dt, EulerStage<T, false>{}, EulerSrc<T, false>{}, W);
    }
  }
  if (c->profile) pa_profile_stop(c, 0);
  PA_HIP(c, hipGetLastError());
  return pa_bc_apply_auto<T>(c, out, false);
}

// pa_rk_march_vel: the buffer rotation of rk_march_t (order 1: the ping-pong of two buffers, b2 is not touched), a BC fill
// behind every step and stage
template <typename T>
static int rk_march_vel_t(pa_ctx* c, T* b0, T* b1, T* b2, int order, int kind, const pa_velocity* vel, double nu, double dt,
                          int64_t nsteps, int* final, const pa_source* src) {
  const double st2[1][2] = {{0.5, 0.5}};
  const double st3[2][2] = {{3.0 / 4.0, 1.0 / 4.0}, {1.0 / 3.0, 2.0 / 3.0}};
  const double (*st)[2] = order == 2 ? st2 : st3;
  T* buf[3] = {b0, b1, b2};
  int base = 0, wa = 1, wb = 2;
  for (int64_t s = 0; s < nsteps; ++s) {
    int rc = euler_vel_t<T>(c, buf[base], buf[wa], kind, vel, nu, dt, nullptr, 0.0, 0.0, src);
    if (rc) return rc;
    int cur = wa, free_ = wb;
    for (int q = 0; q < order - 1; ++q) {
      rc = euler_vel_t<T>(c, buf[cur], buf[free_], kind, vel, nu, dt, buf[base], st[q][0], st[q][1], src);
      if (rc) return rc;
      std::swap(cur, free_);
    }
    const int old = base;
    base = cur; wa = old; wb = free_;
  }
  *final = base;
  return PA_OK;
}

// pa_momentum_march: rk_march_vel_t's rotation over (ncomp, ncell) buffers.  A stage computes every component from the SAME
// input vector: component q of `in` goes to component q of `out` with component q's BC values in the bound list (types, order
// and dxf stay), advected by the frozen velocity `fz` or, fz null, by the input vector itself -- internal axis ia carries
// component ia - (3 - ndim).  The bound list's values are restored on every way out.
template <typename T>
static int momentum_march_t(pa_ctx* c, T* b0, T* b1, T* b2, int ncomp, int order, int kind, const pa_velocity* fz, double nu,
                            double dt, int64_t nsteps, int* final, const pa_source* src, const pa_bc_values* bcv) {
  const double st2[1][2] = {{0.5, 0.5}};
  const double st3[2][2] = {{3.0 / 4.0, 1.0 / 4.0}, {1.0 / 3.0, 2.0 / 3.0}};
  const double (*st)[2] = order == 2 ? st2 : st3;
  const int64_t nc = c->G.ncell;
  const int sh = 3 - c->ndim;
  HostBC saved[6];
  for (int f = 0; f < 6; ++f) saved[f] = c->bc[f];
  auto stage = [&](const T* in, T* out, const T* phi0, double c0, double c1) -> int {
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
      if (int rc = euler_vel_t<T>(c, in + q * nc, out + q * nc, kind, &vi, nu, dt, phi0 ? phi0 + q * nc : nullptr, c0, c1, sq,
                                  fz ? -1 : q + sh))
        return rc;
    }
    return PA_OK;
  };
  T* buf[3] = {b0, b1, b2};
  int base = 0, wa = 1, wb = 2, rc = PA_OK;
  for (int64_t s = 0; s < nsteps && !rc; ++s) {
    rc = stage(buf[base], buf[wa], nullptr, 0.0, 0.0);
    int cur = wa, free_ = wb;
    for (int q = 0; q < order - 1 && !rc; ++q) {
      rc = stage(buf[cur], buf[free_], buf[base], st[q][0], st[q][1]);
      std::swap(cur, free_);
    }
    const int old = base;
    base = cur; wa = old; wb = free_;
  }
  for (int f = 0; f < 6; ++f) c->bc[f] = saved[f];
  if (!rc) *final = base;
  return rc;
}

// ---- vector steps of the host-stepped solver loops (pyapes_amd/solver/host_stepped.py) ------------------------------
// out = y + a x, the product rounded before the sum (torch: y + a * x; "y - a x" is the same bits with -a)
template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_vec_axpy(T* __restrict__ out, const T* __restrict__ y, T a,
                                                        const T* __restrict__ x, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    T t = a * x[i];
    out[i] = y[i] + t;
  }
}

// partial sums of a.b (diff = 0) or of (a - b)^2 (diff = 1), products rounded in T, summed in double
template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_vec_dot(const T* __restrict__ a, const T* __restrict__ b, int diff, int64_t n,
                                                       double* __restrict__ partials) {
  double s[1] = {0.0};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    T p;
    if (diff) { T d = a[i] - b[i]; p = d * d; } else { p = a[i] * b[i]; }
    s[0] += (double)p;
  }
  pa_block_reduce_store<1>(s, partials);
}

// x <- 0 off the interior set of the bound BC list (the residual lives on S, linalg.py:99-101)
template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_vec_mask_interior(DevGeom G, T* __restrict__ x) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < G.ncell; idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t i, j, k;
    pa_decode(G, idx, i, j, k);
    if (!pa_in_S(G, i, j, k)) x[idx] = (T)0;
  }
}

__global__ void __launch_bounds__(PA_BLOCK) k_vec_dot_final(const double* __restrict__ partials, int nblk, double* __restrict__ out) {
  __shared__ double sm[PA_BLOCK / 64];
  double v = 0.0;
  for (int b = threadIdx.x; b < nblk; b += blockDim.x) v += partials[b];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = sm[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) t += sm[w];
    out[0] = t;
  }
}

// (QUICK marches with a BC fill per step or stage: kind == PA_OP_DIV_UPWIND below)
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

// One launch of pa_rk_march: the Euler step (phi0 null) or a fused stage, in -> out.  *bcl: the march is in the "BC on
// load" form.  The form is decided by the first launch (nlaunch 0); should a later one decline it (an operand the
// vector kernel does not take), `in` gets the fill it was left without and the march goes on in the classic sequence --
// the same bits, since the face values a BC-on-load launch forms are the ones the fill stores.
template <typename T>
static int rk_launch_t(pa_ctx* c, bool* bcl, int64_t nlaunch, T* in, T* out, const T* phi0, double c0, double c1, int kind,
                       double u, const void* u_field, double nu, double dt, const pa_source* src) {
  if (*bcl) {
    const int fr = euler_bcl_t<T>(c, in, out, kind, u, u_field, nu, dt, phi0, c0, c1, src);
    if (fr != 0) return fr < 0 ? fr : PA_OK;
    *bcl = false;
    if (nlaunch > 0) {
      if (int rc = pa_bc_apply_auto<T>(c, in, false)) return rc;
    }
  }
  return euler_t<T>(c, in, out, kind, u, u_field, nu, dt, phi0, c0, c1, src);
}

// self: the field advects itself -- every launch takes its own input buffer as the speed field (pa_rk_march_self)
template <typename T>
static int rk_march_t(pa_ctx* c, T* b0, T* b1, T* b2, int order, int kind, double u, const void* u_field, double nu,
                      double dt, int64_t nsteps, int* final, bool self, const pa_source* src) {
  // the fused stages of a step in Shu-Osher form, after its plain Euler stage: (c0, c1) of c0 phi0 + c1 E(phi_s)
  const double st2[1][2] = {{0.5, 0.5}};
  const double st3[2][2] = {{3.0 / 4.0, 1.0 / 4.0}, {1.0 / 3.0, 2.0 / 3.0}};
  const double (*st)[2] = order == 2 ? st2 : st3;
  T* buf[3] = {b0, b1, b2};
  int base = 0, wa = 1, wb = 2;   // buffer of the step's phi0 and the two free ones
  bool bcl = march_bcl_wanted(c, kind, nsteps);
  int64_t nl = 0;
  for (int64_t s = 0; s < nsteps; ++s) {
    int rc = rk_launch_t<T>(c, &bcl, nl++, buf[base], buf[wa], nullptr, 0.0, 0.0, kind, u, self ? buf[base] : u_field, nu, dt, src);
    if (rc) return rc;
    int cur = wa, free_ = wb;
    for (int q = 0; q < order - 1; ++q) {
      rc = rk_launch_t<T>(c, &bcl, nl++, buf[cur], buf[free_], buf[base], st[q][0], st[q][1], kind, u, self ? buf[cur] : u_field, nu,
                          dt, src);
      if (rc) return rc;
      std::swap(cur, free_);
    }
    // cur holds the new state; the old base and the other work buffer are free
    const int old = base;
    base = cur; wa = old; wb = free_;
  }
  *final = base;
  if (bcl && nsteps > 0) {
    PA_HIP(c, hipGetLastError());
    return pa_bc_apply_auto<T>(c, buf[base], false);
  }
  return PA_OK;
}

extern "C" {

int pa_vec_axpy(pa_ctx* c, void* out, const void* y, double a, const void* x) {
  if (!c || !c->grid_set || !out || !y || !x) return PA_E_STATE;
  PA_HIP(c, hipSetDevice(c->device));
  const int nb = pa_grid_blocks(c->G.ncell);
  if (c->dtype == PA_F64)
    hipLaunchKernelGGL(k_vec_axpy<double>, dim3(nb), dim3(PA_BLOCK), 0, c->stream, (double*)out, (const double*)y, a,
                       (const double*)x, c->G.ncell);
  else
    hipLaunchKernelGGL(k_vec_axpy<float>, dim3(nb), dim3(PA_BLOCK), 0, c->stream, (float*)out, (const float*)y, (float)a,
                       (const float*)x, c->G.ncell);
  PA_HIP(c, hipGetLastError());
  return PA_OK;
}

int pa_vec_mask_interior(pa_ctx* c, void* x) {
  if (!c || !c->grid_set || !x) return PA_E_STATE;
  PA_HIP(c, hipSetDevice(c->device));
  const int nb = pa_grid_blocks(c->G.ncell);
  if (c->dtype == PA_F64) hipLaunchKernelGGL(k_vec_mask_interior<double>, dim3(nb), dim3(PA_BLOCK), 0, c->stream, c->G, (double*)x);
  else hipLaunchKernelGGL(k_vec_mask_interior<float>, dim3(nb), dim3(PA_BLOCK), 0, c->stream, c->G, (float*)x);
  PA_HIP(c, hipGetLastError());
  return PA_OK;
}

int pa_vec_dot(pa_ctx* c, const void* a, const void* b, int diff, double* result) {
  if (!c || !c->grid_set || !a || !b || !result) return PA_E_STATE;
  PA_HIP(c, hipSetDevice(c->device));
  const int nb = pa_grid_blocks(c->G.ncell);
  int rc;
  if ((rc = pa_scratch(c, &c->scr[SCR_PART2], &c->cap[SCR_PART2], (size_t)3 * PA_MAX_GRID * sizeof(double)))) return rc;
  double* part = (double*)c->scr[SCR_PART2];
  if (nb + 1 > 3 * PA_MAX_GRID) { pa_set_err(c, "pa_vec_dot: grid too large for the partials buffer"); return PA_E_STATE; }
  if (c->dtype == PA_F64)
    hipLaunchKernelGGL(k_vec_dot<double>, dim3(nb), dim3(PA_BLOCK), 0, c->stream, (const double*)a, (const double*)b, diff,
                       c->G.ncell, part);
  else
    hipLaunchKernelGGL(k_vec_dot<float>, dim3(nb), dim3(PA_BLOCK), 0, c->stream, (const float*)a, (const float*)b, diff,
                       c->G.ncell, part);
  hipLaunchKernelGGL(k_vec_dot_final, dim3(1), dim3(PA_BLOCK), 0, c->stream, (const double*)part, nb, part + nb);
  PA_HIP(c, hipMemcpyAsync(result, part + nb, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  PA_HIP(c, hipStreamSynchronize(c->stream));
  return PA_OK;
}

int pa_aop(pa_ctx* c, const void* x, void* y, int interior_only) {
  if (!c || !c->grid_set || !c->eq_set) { if (c) pa_set_err(c, "pa_aop: grid/equation not set"); return PA_E_STATE; }
  if (int rc0 = pa_check_eq_applicable(c)) return rc0;
  PA_HIP(c, hipSetDevice(c->device));
  return c->dtype == PA_F64 ? aop_t<double>(c, (const double*)x, (double*)y, interior_only, c->nterms, c->terms)
                            : aop_t<float>(c, (const float*)x, (float*)y, interior_only, c->nterms, c->terms);
}

int pa_rhs_adjust(pa_ctx* c, void* rhs) {
  if (!c || !c->grid_set || !c->eq_set) { if (c) pa_set_err(c, "pa_rhs_adjust: grid/equation not set"); return PA_E_STATE; }
  for (int q = 0; q < c->nterms; ++q)
    if (c->terms[q].kind == PA_OP_DIV_QUICK) { pa_set_err(c, "pa_rhs_adjust: Div quick is explicit-only"); return PA_E_ARG; }
  PA_HIP(c, hipSetDevice(c->device));
  return c->dtype == PA_F64 ? rhs_adjust_t<double>(c, (double*)rhs) : rhs_adjust_t<float>(c, (float*)rhs);
}

int pa_laplacian(pa_ctx* c, const void* x, void* y, int edge) {
  if (!c || !c->grid_set) return PA_E_STATE;
  PA_HIP(c, hipSetDevice(c->device));
  return c->dtype == PA_F64 ? lap_t<double>(c, (const double*)x, (double*)y, edge)
                            : lap_t<float>(c, (const float*)x, (float*)y, edge);
}

int pa_grad(pa_ctx* c, const void* x, void* y, int edge) {
  if (!c || !c->grid_set) return PA_E_STATE;
  PA_HIP(c, hipSetDevice(c->device));
  return c->dtype == PA_F64 ? grad_t<double>(c, (const double*)x, (double*)y, edge)
                            : grad_t<float>(c, (const float*)x, (float*)y, edge);
}

int pa_div(pa_ctx* c, int kind, double u, const void* u_field, const void* x, void* y) {
  if (!c || !c->grid_set) return PA_E_STATE;
  int rc = check_div_kind(c, kind);
  if (rc) return rc;
  PA_HIP(c, hipSetDevice(c->device));
  pa_term t;
  memset(&t, 0, sizeof(t));
  t.kind = kind; t.sign = 1.0; t.u = u; t.u_field = u_field;
  return c->dtype == PA_F64 ? aop_t<double>(c, (const double*)x, (double*)y, 0, 1, &t)
                            : aop_t<float>(c, (const float*)x, (float*)y, 0, 1, &t);
}

int pa_div_edge(pa_ctx* c, double u, const void* u_field, const void* x, void* y) {
  if (!c || !c->grid_set) return PA_E_STATE;
  if (c->ndim != 1) {
    pa_set_err(c, "edge=True Div of a scalar field is 1-D only (the reference raises IndexError, fdc.py:296-303)");
    return PA_E_ARG;
  }
  if (c->G.n2 < 3) { pa_set_err(c, "edge Div needs >= 3 nodes"); return PA_E_ARG; }
  PA_HIP(c, hipSetDevice(c->device));
  pa_term t;
  memset(&t, 0, sizeof(t));
  t.kind = PA_OP_GRAD; t.sign = 1.0;
  if (c->dtype == PA_F64) {
    DevEq<double> E;
    pa_build_eq<double>(c, 1, &t, E);
    hipLaunchKernelGGL(k_edge<double>, dim3(pa_grid_blocks(c->G.ncell)), dim3(PA_BLOCK), 0, c->stream, c->G, E,
                       (const double*)x, (double*)y, c->ndim, 2, (double)u, (const double*)u_field);
  } else {
    DevEq<float> E;
    pa_build_eq<float>(c, 1, &t, E);
    hipLaunchKernelGGL(k_edge<float>, dim3(pa_grid_blocks(c->G.ncell)), dim3(PA_BLOCK), 0, c->stream, c->G, E,
                       (const float*)x, (float*)y, c->ndim, 2, (float)u, (const float*)u_field);
  }
  PA_HIP(c, hipGetLastError());
  return PA_OK;
}

// The source of a pa_*_src call.  NULL or has == 0: *src becomes null and the call is its sibling.  Else slab mode
// (PA_E_STATE), an axisymmetric mesh and a field that overlaps one of the call's buffers (PA_E_ARG) are refused before
// anything is enqueued.
static int check_source(pa_ctx* c, const pa_source** src, const char* who, std::initializer_list<const void*> bufs) {
  if (!*src || !(*src)->has) { *src = nullptr; return PA_OK; }
  if (c->slab || (c->G.n0 != c->G.g0 && c->ndim == 3)) { pa_set_err(c, "%s: a source term is single GPU only (no slabs)", who); return PA_E_STATE; }
  if (c->coord != PA_COORD_XYZ) { pa_set_err(c, "%s: a source term is for xyz meshes (no axisymmetric rows)", who); return PA_E_ARG; }
  const char* f = (const char*)(*src)->field;
  if (!f) return PA_OK;
  const size_t bytes = (size_t)c->G.ncell * (c->dtype == PA_F64 ? 8 : 4);
  for (const void* b : bufs)
    if (b && f < (const char*)b + bytes && (const char*)b < f + bytes) {
      pa_set_err(c, "%s: the source field must not be one of the call's buffers", who);
      return PA_E_ARG;
    }
  return PA_OK;
}

// The velocity of a pa_*_vel call: the refusals of the header, made before anything is enqueued, and the velocity by INTERNAL
// axis in *vi (a d-dimensional mesh occupies the last d internal axes; the others carry a zero speed that is never read).
static int check_velocity(pa_ctx* c, const pa_velocity* vel, pa_velocity* vi, int kind, const pa_source* src, const char* who,
                          std::initializer_list<const void*> bufs) {
  if (!vel || !vel->has) { pa_set_err(c, "%s: a velocity is needed (vel == NULL or has == 0)", who); return PA_E_ARG; }
  if (kind == PA_OP_DIV_UPWIND_COMPAT) { pa_set_err(c, "%s: the literal upwind form takes no velocity", who); return PA_E_ARG; }
  if (c->slab || (c->G.n0 != c->G.g0 && c->ndim == 3)) { pa_set_err(c, "%s: a velocity is single GPU only (no slabs)", who); return PA_E_STATE; }
  if (c->coord != PA_COORD_XYZ) { pa_set_err(c, "%s: a velocity is for xyz meshes (no axisymmetric rows)", who); return PA_E_ARG; }
  memset(vi, 0, sizeof(*vi));
  vi->has = 1;
  const size_t bytes = (size_t)c->G.ncell * (c->dtype == PA_F64 ? 8 : 4);
  const char* sf = src ? (const char*)src->field : nullptr;
  for (int a = 0; a < c->ndim; ++a) {
    const int ia = a + 3 - c->ndim;
    vi->value[ia] = vel->value[a];
    vi->field[ia] = vel->field[a];
    const char* f = (const char*)vel->field[a];
    if (!f) continue;
    bool hit = sf && f < sf + bytes && sf < f + bytes;
    for (const void* b : bufs) hit = hit || (b && f < (const char*)b + bytes && (const char*)b < f + bytes);
    if (hit) { pa_set_err(c, "%s: a velocity field must not be one of the call's buffers or the source field", who); return PA_E_ARG; }
  }
  return PA_OK;
}

int pa_euler_step_vel(pa_ctx* c, const void* in, void* out, int kind, const pa_velocity* vel, double nu, double dt,
                      const pa_source* src) {
  if (!c || !c->grid_set) return PA_E_STATE;
  int rc = check_div_kind(c, kind, "pa_euler_step_vel");
  if (rc) return rc;
  if (!in || !out || in == out) { pa_set_err(c, "pa_euler_step_vel: in-place step is not allowed"); return PA_E_ARG; }
  if ((rc = check_source(c, &src, "pa_euler_step_vel", {in, out}))) return rc;
  pa_velocity vi;
  if ((rc = check_velocity(c, vel, &vi, kind, src, "pa_euler_step_vel", {in, out}))) return rc;
  PA_HIP(c, hipSetDevice(c->device));
  return c->dtype == PA_F64 ? euler_vel_t<double>(c, (const double*)in, (double*)out, kind, &vi, nu, dt, nullptr, 0.0, 0.0, src)
                            : euler_vel_t<float>(c, (const float*)in, (float*)out, kind, &vi, nu, dt, nullptr, 0.0, 0.0, src);
}

int pa_rk_stage_vel(pa_ctx* c, const void* phi, const void* phi0, void* out, double c0, double c1, int kind,
                    const pa_velocity* vel, double nu, double dt, const pa_source* src) {
  if (!c || !c->grid_set) return PA_E_STATE;
  int rc = check_div_kind(c, kind, "pa_rk_stage_vel");
  if (rc) return rc;
  if (!phi || !phi0 || !out || out == phi || out == phi0) {
    pa_set_err(c, "pa_rk_stage_vel: out must be a buffer of its own (not phi, not phi0)");
    return PA_E_ARG;
  }
  if ((rc = check_source(c, &src, "pa_rk_stage_vel", {phi, phi0, out}))) return rc;
  pa_velocity vi;
  if ((rc = check_velocity(c, vel, &vi, kind, src, "pa_rk_stage_vel", {phi, phi0, out}))) return rc;
  PA_HIP(c, hipSetDevice(c->device));
  return c->dtype == PA_F64
             ? euler_vel_t<double>(c, (const double*)phi, (double*)out, kind, &vi, nu, dt, (const double*)phi0, c0, c1, src)
             : euler_vel_t<float>(c, (const float*)phi, (float*)out, kind, &vi, nu, dt, (const float*)phi0, c0, c1, src);
}

int pa_rk_march_vel(pa_ctx* c, void* phi, void* w1, void* w2, int order, int kind, const pa_velocity* vel, double nu,
                    double dt, int64_t nsteps, int* final, const pa_source* src) {
  if (!c || !c->grid_set) return PA_E_STATE;
  if (order < 1 || order > 3) { pa_set_err(c, "pa_rk_march_vel: order %d (1, 2 or 3)", order); return PA_E_ARG; }
  int rc = check_div_kind(c, kind, "pa_rk_march_vel");
  if (rc) return rc;
  if (!phi || !w1 || !final || phi == w1 || nsteps < 0 || (order > 1 && (!w2 || phi == w2 || w1 == w2))) {
    pa_set_err(c, "pa_rk_march_vel: distinct buffers (two for order 1, else three), a place for the result index and "
                  "nsteps >= 0 are needed");
    return PA_E_ARG;
  }
  if (order == 1) w2 = nullptr;
  if ((rc = check_source(c, &src, "pa_rk_march_vel", {phi, w1, w2}))) return rc;
  pa_velocity vi;
  if ((rc = check_velocity(c, vel, &vi, kind, src, "pa_rk_march_vel", {phi, w1, w2}))) return rc;
  PaRange range_("pyapes march in a velocity field");
  PA_HIP(c, hipSetDevice(c->device));
  return c->dtype == PA_F64
             ? rk_march_vel_t<double>(c, (double*)phi, (double*)w1, (double*)w2, order, kind, &vi, nu, dt, nsteps, final, src)
             : rk_march_vel_t<float>(c, (float*)phi, (float*)w1, (float*)w2, order, kind, &vi, nu, dt, nsteps, final, src);
}

int pa_momentum_march(pa_ctx* c, void* U, void* w1, void* w2, int ncomp, int order, int kind, const pa_velocity* frozen, double nu,
                      double dt, int64_t nsteps, int* final, const pa_source* src, const pa_bc_values* bcv) {
  if (!c || !c->grid_set) return PA_E_STATE;
  const char* who = "pa_momentum_march";
  if (order < 1 || order > 3) { pa_set_err(c, "%s: order %d (1, 2 or 3)", who, order); return PA_E_ARG; }
  if (c->slab || (c->G.n0 != c->G.g0 && c->ndim == 3)) { pa_set_err(c, "%s: single GPU only (no slabs)", who); return PA_E_STATE; }
  if (c->coord != PA_COORD_XYZ) { pa_set_err(c, "%s: for xyz meshes (no axisymmetric rows)", who); return PA_E_ARG; }
  if (c->ndim < 2 || ncomp != c->ndim) {
    pa_set_err(c, "%s: one component per mesh axis on a 2-D or 3-D mesh (%d components, %d axes)", who, ncomp, c->ndim);
    return PA_E_ARG;
  }
  if (kind == PA_OP_DIV_UPWIND_COMPAT) { pa_set_err(c, "%s: the literal upwind form takes no velocity", who); return PA_E_ARG; }
  int rc = check_div_kind(c, kind, who);
  if (rc) return rc;
  if (order == 1) w2 = nullptr;
  if (!U || !w1 || !final || !bcv || nsteps < 0 || (order > 1 && !w2)) {
    pa_set_err(c, "%s: buffers (two for order 1, else three), a place for the result index, BC values and nsteps >= 0 are needed", who);
    return PA_E_ARG;
  }
  const size_t cbytes = (size_t)c->G.ncell * (c->dtype == PA_F64 ? 8 : 4), vbytes = cbytes * (size_t)ncomp;
  const void* bufs[3] = {U, w1, w2};
  auto hits = [&](const void* p, size_t bytes) {   // [p, p + bytes) against the three vector buffers
    for (const void* b : bufs)
      if (b && p && (const char*)p < (const char*)b + vbytes && (const char*)b < (const char*)p + bytes) return true;
    return false;
  };
  for (int i = 0; i < 3; ++i)
    for (int j = i + 1; j < 3; ++j)
      if (bufs[i] && bufs[j] && (const char*)bufs[i] < (const char*)bufs[j] + vbytes && (const char*)bufs[j] < (const char*)bufs[i] + vbytes) {
        pa_set_err(c, "%s: the buffers must not overlap", who);
        return PA_E_ARG;
      }
  pa_velocity vi;
  if (frozen) {
    if (!frozen->has) { pa_set_err(c, "%s: a frozen velocity with has == 0", who); return PA_E_ARG; }
    memset(&vi, 0, sizeof(vi));
    vi.has = 1;
    for (int a = 0; a < c->ndim; ++a) {
      vi.value[a + 3 - c->ndim] = frozen->value[a];
      vi.field[a + 3 - c->ndim] = frozen->field[a];
      if (hits(frozen->field[a], cbytes)) { pa_set_err(c, "%s: a frozen velocity field must not overlap a buffer of the call", who); return PA_E_ARG; }
    }
  }
  if (src)
    for (int q = 0; q < ncomp; ++q)
      if (src[q].has && hits(src[q].field, cbytes)) { pa_set_err(c, "%s: a source field must not overlap a buffer of the call", who); return PA_E_ARG; }
  {
    const int64_t n[3] = {c->G.n0, c->G.n1, c->G.n2};
    for (int q = 0; q < ncomp; ++q)
      for (int f = 0; f < 2 * c->ndim; ++f) {
        const size_t fbytes = cbytes / (size_t)n[(f >> 1) + 3 - c->ndim];
        if (hits(bcv[q].vals[f], fbytes)) { pa_set_err(c, "%s: a BC face array must not overlap a buffer of the call", who); return PA_E_ARG; }
      }
  }
  PaRange range_("pyapes momentum march");
  PA_HIP(c, hipSetDevice(c->device));
  return c->dtype == PA_F64
             ? momentum_march_t<double>(c, (double*)U, (double*)w1, (double*)w2, ncomp, order, kind, frozen ? &vi : nullptr, nu, dt, nsteps, final, src, bcv)
             : momentum_march_t<float>(c, (float*)U, (float*)w1, (float*)w2, ncomp, order, kind, frozen ? &vi : nullptr, nu, dt, nsteps, final, src, bcv);
}

int pa_euler_step_src(pa_ctx* c, const void* in, void* out, int kind, double u, const void* u_field, double nu, double dt,
                      const pa_source* src) {
  if (!c || !c->grid_set) return PA_E_STATE;
  int rc = check_div_kind(c, kind, "pa_euler_step");
  if (rc) return rc;
  if (in == out) { pa_set_err(c, "pa_euler_step: in-place step is not allowed"); return PA_E_ARG; }
  if ((rc = check_source(c, &src, "pa_euler_step_src", {in, out, u_field}))) return rc;
  PA_HIP(c, hipSetDevice(c->device));
  return c->dtype == PA_F64
             ? euler_t<double>(c, (const double*)in, (double*)out, kind, u, u_field, nu, dt, nullptr, 0.0, 0.0, src)
             : euler_t<float>(c, (const float*)in, (float*)out, kind, u, u_field, nu, dt, nullptr, 0.0, 0.0, src);
}

int pa_euler_step(pa_ctx* c, const void* in, void* out, int kind, double u, const void* u_field, double nu,
                  double dt) {
  return pa_euler_step_src(c, in, out, kind, u, u_field, nu, dt, nullptr);
}

// self: every step takes its own input buffer as the speed field (order 1 of pa_rk_march_self)
static int euler_march_impl(pa_ctx* c, void* phi, void* tmp, int kind, double u, const void* u_field_, double nu, double dt,
                            int64_t nsteps, bool self, const pa_source* src) {
  int rc;
  PaRange range_("pyapes explicit Euler march");
  PA_HIP(c, hipSetDevice(c->device));
  void* buf[2] = {phi, tmp};
  bool bcl = march_bcl_wanted(c, kind, nsteps);
  for (int64_t s = 0; s < nsteps; ++s) {
    const void* u_field = self ? buf[s & 1] : u_field_;
    if (bcl) {
      const int fr = c->dtype == PA_F64
                         ? euler_bcl_t<double>(c, (const double*)buf[s & 1], (double*)buf[(s + 1) & 1], kind, u, u_field, nu, dt, nullptr, 0.0, 0.0, src)
                         : euler_bcl_t<float>(c, (const float*)buf[s & 1], (float*)buf[(s + 1) & 1], kind, u, u_field, nu, dt, nullptr, 0.0, 0.0, src);
      if (fr < 0) return fr;
      if (fr > 0) continue;
      if (s > 0) { pa_set_err(c, "pa_euler_march: the BC-on-load step declined in the middle of a march"); return PA_E_STATE; }
      bcl = false;   // not for k_sf (row length, alignment ...): the classic sequence from the first step on
    }
    rc = c->dtype == PA_F64
             ? euler_t<double>(c, (const double*)buf[s & 1], (double*)buf[(s + 1) & 1], kind, u, u_field, nu, dt, nullptr, 0.0, 0.0, src)
             : euler_t<float>(c, (const float*)buf[s & 1], (float*)buf[(s + 1) & 1], kind, u, u_field, nu, dt, nullptr, 0.0, 0.0, src);
    if (rc) return rc;
  }
  if (bcl && nsteps > 0) {
    PA_HIP(c, hipGetLastError());
    return c->dtype == PA_F64 ? pa_bc_apply_auto<double>(c, (double*)buf[nsteps & 1], false)
                              : pa_bc_apply_auto<float>(c, (float*)buf[nsteps & 1], false);
  }
  return PA_OK;
}

int pa_euler_march_src(pa_ctx* c, void* phi, void* tmp, int kind, double u, const void* u_field, double nu, double dt,
                       int64_t nsteps, const pa_source* src) {
  if (!c || !c->grid_set) return PA_E_STATE;
  int rc = check_div_kind(c, kind, "pa_euler_march");
  if (rc) return rc;
  if (phi == tmp || nsteps < 0) { pa_set_err(c, "pa_euler_march: bad buffers / step count"); return PA_E_ARG; }
  if ((rc = check_source(c, &src, "pa_euler_march_src", {phi, tmp, u_field}))) return rc;
  return euler_march_impl(c, phi, tmp, kind, u, u_field, nu, dt, nsteps, false, src);
}

int pa_euler_march(pa_ctx* c, void* phi, void* tmp, int kind, double u, const void* u_field, double nu, double dt,
                   int64_t nsteps) {
  return pa_euler_march_src(c, phi, tmp, kind, u, u_field, nu, dt, nsteps, nullptr);
}

int pa_rk_stage_src(pa_ctx* c, const void* phi, const void* phi0, void* out, double c0, double c1, int kind, double u,
                    const void* u_field, double nu, double dt, const pa_source* src) {
  if (!c || !c->grid_set) return PA_E_STATE;
  int rc = check_div_kind(c, kind, "pa_rk_stage");
  if (rc) return rc;
  if (!phi || !phi0 || !out || out == phi || out == phi0) {
    pa_set_err(c, "pa_rk_stage: out must be a buffer of its own (not phi, not phi0)");
    return PA_E_ARG;
  }
  if (c->slab || (c->G.n0 != c->G.g0 && c->ndim == 3)) { pa_set_err(c, "pa_rk_stage: single GPU only (no slab stages)"); return PA_E_STATE; }
  if ((rc = check_source(c, &src, "pa_rk_stage_src", {phi, phi0, out, u_field}))) return rc;
  PA_HIP(c, hipSetDevice(c->device));
  return c->dtype == PA_F64
             ? euler_t<double>(c, (const double*)phi, (double*)out, kind, u, u_field, nu, dt, (const double*)phi0, c0, c1, src)
             : euler_t<float>(c, (const float*)phi, (float*)out, kind, u, u_field, nu, dt, (const float*)phi0, c0, c1, src);
}

int pa_rk_stage(pa_ctx* c, const void* phi, const void* phi0, void* out, double c0, double c1, int kind, double u,
                const void* u_field, double nu, double dt) {
  return pa_rk_stage_src(c, phi, phi0, out, c0, c1, kind, u, u_field, nu, dt, nullptr);
}

int pa_rk_march_src(pa_ctx* c, void* phi, void* w1, void* w2, int order, int kind, double u, const void* u_field, double nu,
                    double dt, int64_t nsteps, int* final, const pa_source* src) {
  if (!c || !c->grid_set) return PA_E_STATE;
  if (order < 1 || order > 3) { pa_set_err(c, "pa_rk_march: order %d (1, 2 or 3)", order); return PA_E_ARG; }
  int rc = check_div_kind(c, kind, "pa_rk_march");
  if (rc) return rc;
  if (!phi || !w1 || !w2 || !final || phi == w1 || phi == w2 || w1 == w2 || nsteps < 0) {
    pa_set_err(c, "pa_rk_march: three distinct buffers, a place for the result index and nsteps >= 0 are needed");
    return PA_E_ARG;
  }
  if (c->slab || (c->G.n0 != c->G.g0 && c->ndim == 3)) { pa_set_err(c, "pa_rk_march: single GPU only (no slab stages)"); return PA_E_STATE; }
  if ((rc = check_source(c, &src, "pa_rk_march_src", {phi, w1, w2, u_field}))) return rc;
  if (order == 1) {   // plain Euler: the march as it is
    rc = pa_euler_march_src(c, phi, w1, kind, u, u_field, nu, dt, nsteps, src);
    if (!rc) *final = (int)(nsteps & 1);
    return rc;
  }
  PaRange range_("pyapes SSP Runge-Kutta march");
  PA_HIP(c, hipSetDevice(c->device));
  return c->dtype == PA_F64
             ? rk_march_t<double>(c, (double*)phi, (double*)w1, (double*)w2, order, kind, u, u_field, nu, dt, nsteps, final, false, src)
             : rk_march_t<float>(c, (float*)phi, (float*)w1, (float*)w2, order, kind, u, u_field, nu, dt, nsteps, final, false, src);
}

int pa_rk_march(pa_ctx* c, void* phi, void* w1, void* w2, int order, int kind, double u, const void* u_field, double nu,
                double dt, int64_t nsteps, int* final) {
  return pa_rk_march_src(c, phi, w1, w2, order, kind, u, u_field, nu, dt, nsteps, final, nullptr);
}

int pa_rk_march_self_src(pa_ctx* c, void* phi, void* w1, void* w2, int order, int kind, double nu, double dt, int64_t nsteps,
                         int* final, const pa_source* src) {
  if (!c || !c->grid_set) return PA_E_STATE;
  if (order < 1 || order > 3) { pa_set_err(c, "pa_rk_march_self: order %d (1, 2 or 3)", order); return PA_E_ARG; }
  int rc = check_div_kind(c, kind, "pa_rk_march_self");
  if (rc) return rc;
  if (!phi || !w1 || !final || phi == w1 || nsteps < 0 || (order > 1 && (!w2 || phi == w2 || w1 == w2))) {
    pa_set_err(c, "pa_rk_march_self: distinct buffers (two for order 1, else three), a place for the result index and "
                  "nsteps >= 0 are needed");
    return PA_E_ARG;
  }
  if (c->slab || (c->G.n0 != c->G.g0 && c->ndim == 3)) { pa_set_err(c, "pa_rk_march_self: single GPU only (no slab stages)"); return PA_E_STATE; }
  if ((rc = check_source(c, &src, "pa_rk_march_self_src", {phi, w1, order > 1 ? w2 : nullptr}))) return rc;
  if (order == 1) {   // plain Euler, the speed ping-pongs with the field
    rc = euler_march_impl(c, phi, w1, kind, 0.0, nullptr, nu, dt, nsteps, true, src);
    if (!rc) *final = (int)(nsteps & 1);
    return rc;
  }
  PaRange range_("pyapes SSP Runge-Kutta march, self-advected");
  PA_HIP(c, hipSetDevice(c->device));
  return c->dtype == PA_F64
             ? rk_march_t<double>(c, (double*)phi, (double*)w1, (double*)w2, order, kind, 0.0, nullptr, nu, dt, nsteps, final, true, src)
             : rk_march_t<float>(c, (float*)phi, (float*)w1, (float*)w2, order, kind, 0.0, nullptr, nu, dt, nsteps, final, true, src);
}

int pa_rk_march_self(pa_ctx* c, void* phi, void* w1, void* w2, int order, int kind, double nu, double dt, int64_t nsteps,
                     int* final) {
  return pa_rk_march_self_src(c, phi, w1, w2, order, kind, nu, dt, nsteps, final, nullptr);
}

}  // extern "C"
