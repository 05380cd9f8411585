// pa_sfn_kernel.h -- k_sfn, the sibling of k_sf (pa_sf_kernel.h) for the explicit Euler step / Runge-Kutta stage with a
// DIFFUSIVITY FIELD: div(nu grad phi), nu per node, in the place of nu * lap(phi), with the upwind Div of ONE SCALAR speed
// (u == 0: pure heterogeneous diffusion).  On the interior set, per axis a, every operation rounded on its own (-ffp-contract=off):
//     nup = nu[+1]_a + nu;  num = nu + nu[-1]_a;  fp = x[+1]_a - x;  fm = x - x[-1]_a
//     t = nup*fp;  s = num*fm;  t = t - s;  t = t*w_a;  d = d + t            (d starts at +0; w_a = 0.5 * (ih_a * ih_a))
//     adv as the upwind step of k_sf forms it with both halves (US 0);   a = d - adv;  a = dt*a;  v = phi + a
// operation for operation what the NU instantiations of the generic k_euler compute (pa_march.hip pa_nu_term): the same bits
// (tests/test_gpu_nu.py).
//
// It is the first step kernel with a SECOND field that has stencil reach: nu is needed at j +- 1, i +- 1 and k +- 1 exactly as
// phi is.  k_sfn marches BOTH fields the way k_sf marches one -- every wave on its own, no LDS, no barrier: per field four
// planes of the wave's RJ rows in registers (behind / current / ahead / loading, compile-time slots), the rows above / below
// the row block (Hu / Hd) and the two edge cells of every row (He) loaded two planes ahead, k +- 1 across lanes by DPP.  Both
// fields share every offset: one set of address registers.  That doubles the plane registers (fp32, two rows: 72 -> 144), which
// is why there is a two-row form only, and why this is a kernel of its own: k_sf's instantiations stay the code they were.
// A sibling and not `nu` in LDS: staging a plane of nu behind a workgroup barrier is what k_cg3d does, and the Euler step ran
// at 0.49 of the roofline there (pa_sf_kernel.h, head).
//
// The wave geometry, the XCD-aware tile order, the clamped / wrapped unconditional loads and the sched_barrier that keeps the
// loads of plane q + 2 above the arithmetic of plane q are k_sf's; see there for why each is the way it is.  Planes beyond the
// ends of axis 0 wrap around for both fields (one GPU only: pa_tile3d_step declines slabs for this term), as the generic
// kernel's indices do.  Like k_sf the kernel writes the step's value at EVERY node: it takes only launches behind which the BC
// fill rewrites every node outside the interior set (sf_applies, out_all).
// STG: the stage of an SSP Runge-Kutta step, c0 * phi0 + c1 * e stored in the place of e, phi0 read at the cell (as k_sf).
#pragma once
#include "pa_sf_kernel.h"

template <typename T, int RJ, bool STG>
__global__ void __launch_bounds__(256) k_sfn(Cg3dArgs<T> A) {
  constexpr int VEC = VecOf<T>::N;
  typedef T V __attribute__((ext_vector_type(VEC)));
  constexpr int TJ = 4 * RJ, TK = 64 * VEC;
  const DevGeom& G = A.G;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int vb = pa_xcd_remap(blockIdx.x, gridDim.x);
  const int tiles = A.tiles_j * A.tiles_k;
  const int chunk = vb / tiles, tl = vb - chunk * tiles;
  const int tjb = tl / A.tiles_k, tkb = tl - tjb * A.tiles_k;
  const int n0 = (int)G.n0, n1 = (int)G.n1, n2 = (int)G.n2;
  const int i0 = (int)((int64_t)chunk * n0 / A.chunks), i1 = (int)((int64_t)(chunk + 1) * n0 / A.chunks);
  const int CI = i1 - i0;
  const int j0 = tjb * TJ + wv * RJ, k0 = tkb * TK;
  auto wrap = [](int v, int n) { v %= n; return v < 0 ? v + n : v; };

  // ---- per-thread geometry: RJ rows x VEC columns, as 32-bit byte offsets inside a plane (shared by phi, nu, phi0) ----
  const int kg = k0 + lane * VEC;
  const int kc = wrap(kg, n2);
  const bool kvalid = kg < n2;
  unsigned off[RJ], offe[RJ];
  const int ecol = lane == 63 ? wrap(k0 + TK, n2) : wrap(k0 - 1, n2);   // lane 0: cell left of the tile, 63: right
  bool rowOk[RJ];
#pragma unroll
  for (int jj = 0; jj < RJ; ++jj) {
    const int jg = j0 + jj;
    const unsigned ro = (unsigned)wrap(jg, n1) * (unsigned)n2;
    off[jj] = (ro + (unsigned)kc) * (unsigned)sizeof(T);
    offe[jj] = (ro + (unsigned)ecol) * (unsigned)sizeof(T);
    rowOk[jj] = kvalid && jg < n1;
  }
  const unsigned offu = ((unsigned)wrap(j0 - 1, n1) * (unsigned)n2 + (unsigned)kc) * (unsigned)sizeof(T);
  const unsigned offd = ((unsigned)wrap(j0 + RJ, n1) * (unsigned)n2 + (unsigned)kc) * (unsigned)sizeof(T);
  const size_t pstride = (size_t)G.s0 * sizeof(T);
  // byte offset of plane ii of either field, wrapped around the ends of axis 0: uniform and branch-free (k_sf `plane`)
  auto poff = [&](int ii) -> size_t {
    const int ic = ii < 0 ? ii + n0 : (ii >= n0 ? ii - n0 : ii);
    return (size_t)(unsigned)ic * pstride;
  };
  typedef const char __attribute__((address_space(1))) * gcptr;
  const uintptr_t bx = (uintptr_t)A.d.p, bn = (uintptr_t)A.nu_f;

  const V uplC = (V)(A.u < (T)0 ? (T)0 : A.u), umiC = (V)(A.u > (T)0 ? (T)0 : A.u);

  // ---- register planes of the two fields: slot of chunk-relative plane q is (q + 1) & 3; halo slot q & 3 -----------------
  V P[4][RJ], N[4][RJ];
  V Hu[4], Hd[4], NHu[4], NHd[4];
  T He[4][RJ], NHe[4][RJ];

  auto load_own = [&](auto SLOT, int ii) {
    constexpr int s = decltype(SLOT)::value;
    const size_t po = poff(ii);
    gcptr p = (gcptr)(bx + po), q = (gcptr)(bn + po);
#pragma unroll
    for (int jj = 0; jj < RJ; ++jj) {
      P[s][jj] = *reinterpret_cast<const V __attribute__((address_space(1)))*>(p + off[jj]);
      N[s][jj] = *reinterpret_cast<const V __attribute__((address_space(1)))*>(q + off[jj]);
    }
  };
  auto load_halo = [&](auto SLOT, int ii) {
    constexpr int s = decltype(SLOT)::value;
    const size_t po = poff(ii);
    gcptr p = (gcptr)(bx + po), q = (gcptr)(bn + po);
    Hu[s] = *reinterpret_cast<const V __attribute__((address_space(1)))*>(p + offu);
    Hd[s] = *reinterpret_cast<const V __attribute__((address_space(1)))*>(p + offd);
    NHu[s] = *reinterpret_cast<const V __attribute__((address_space(1)))*>(q + offu);
    NHd[s] = *reinterpret_cast<const V __attribute__((address_space(1)))*>(q + offd);
#pragma unroll
    for (int jj = 0; jj < RJ; ++jj) {
      He[s][jj] = *reinterpret_cast<const T __attribute__((address_space(1)))*>(p + offe[jj]);
      NHe[s][jj] = *reinterpret_cast<const T __attribute__((address_space(1)))*>(q + offe[jj]);
    }
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  using I3 = std::integral_constant<int, 3>;

  // prologue: planes -1, 0, 1 of the chunk and the halo of planes 0, 1
  load_own(I0{}, i0 - 1);
  load_own(I1{}, i0);
  load_halo(I0{}, i0);
  load_own(I2{}, i0 + 1);
  load_halo(I1{}, i0 + 1 < i1 ? i0 + 1 : i1 - 1);

  // one plane: C = q & 3 (q = chunk-relative plane index); slots behind C, current C+1, ahead C+2, loading C+3
  auto step = [&](auto CC, int q) {
    constexpr int C = decltype(CC)::value;
    constexpr int SB = C & 3, SC = (C + 1) & 3, SA = (C + 2) & 3, SL = (C + 3) & 3, HC = C & 3, HN = (C + 2) & 3;
    const int ii = i0 + q;
    V Z[STG ? RJ : 1];   // STG: phi0 of THIS plane, issued in front of the loads of plane q + 2 (k_sf)
    if constexpr (STG) {
      gcptr pz = (gcptr)((uintptr_t)A.stg_phi0 + (size_t)(unsigned)ii * pstride);
#pragma unroll
      for (int jj = 0; jj < RJ; ++jj) Z[jj] = *reinterpret_cast<const V __attribute__((address_space(1)))*>(pz + off[jj]);
    }
    load_own(std::integral_constant<int, SL>{}, ii + 2 <= i1 ? ii + 2 : i1);
    load_halo(std::integral_constant<int, HN>{}, ii + 2 < i1 ? ii + 2 : i1 - 1);
    __builtin_amdgcn_sched_barrier(0);   // keep the loads HERE (k_sf: the software pipeline)

    char* const po = (char*)A.out + (size_t)ii * pstride;
#pragma unroll
    for (int jj = 0; jj < RJ; ++jj) {
      const V xc = P[SC][jj], nc = N[SC][jj];
      V up, dn, nu_, nd_;   // rows j-1 / j+1 of the two fields
      if (jj > 0) { up = P[SC][jj - 1]; nu_ = N[SC][jj - 1]; } else { up = Hu[HC]; nu_ = NHu[HC]; }
      if (jj < RJ - 1) { dn = P[SC][jj + 1]; nd_ = N[SC][jj + 1]; } else { dn = Hd[HC]; nd_ = NHd[HC]; }
      // k-1 / k+1: inside the lane's vector, across lanes by DPP (lane 0 / 63 keep the tile's edge cell)
      V xpk, xmk, npk, nmk;
      const T xFromPrev = SfBits<T>::prev(xc[VEC - 1], He[HC][jj]);
      const T xFromNext = SfBits<T>::next(xc[0], He[HC][jj]);
      const T nFromPrev = SfBits<T>::prev(nc[VEC - 1], NHe[HC][jj]);
      const T nFromNext = SfBits<T>::next(nc[0], NHe[HC][jj]);
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        xpk[v] = (v < VEC - 1) ? xc[v + 1 < VEC ? v + 1 : v] : xFromNext;
        xmk[v] = (v > 0) ? xc[v > 0 ? v - 1 : 0] : xFromPrev;
        npk[v] = (v < VEC - 1) ? nc[v + 1 < VEC ? v + 1 : v] : nFromNext;
        nmk[v] = (v > 0) ? nc[v > 0 ? v - 1 : 0] : nFromPrev;
      }
      const V xp3[3] = {P[SA][jj], dn, xpk}, xm3[3] = {P[SB][jj], up, xmk};
      const V np3[3] = {N[SA][jj], nd_, npk}, nm3[3] = {N[SB][jj], nu_, nmk};
      V d = (V)(T)0, adv = (V)(T)0;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        V nup = np3[a] + nc;
        V num = nc + nm3[a];
        V fp = xp3[a] - xc;
        V fm = xc - xm3[a];
        V t = nup * fp;
        V s = num * fm;
        t = t - s;
        t = t * A.nu_w[a];
        d = d + t;
        // the upwind term of the same axis: fm / fp are its backward / forward differences
        V ta = uplC * fm;
        V m2 = umiC * fp;
        ta = ta + m2;
        ta = ta * A.ih[a];
        adv = adv + ta;
      }
      V qv = d - adv;
      qv = A.p1 * qv;
      V res = xc + qv;
      if constexpr (STG) {
        V t0 = A.stg_c0 * Z[jj];
        V t1 = A.stg_c1 * res;
        res = t0 + t1;
      }
      if (rowOk[jj]) *reinterpret_cast<V*>(po + off[jj]) = res;
    }
  };

  for (int q = 0; q < CI; q += 4) {
    step(I0{}, q);
    if (q + 1 < CI) step(I1{}, q + 1);
    if (q + 2 < CI) step(I2{}, q + 2);
    if (q + 3 < CI) step(I3{}, q + 3);
  }
}
