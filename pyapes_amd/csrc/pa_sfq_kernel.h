// pa_sfq_kernel.h -- k_sfq, the explicit Euler step (and the fused SSP Runge-Kutta stage) with the QUICK advection term,
// PA_OP_DIV_QUICK: the sibling of k_sf PHASE 3 (pa_sf_kernel.h) for a stencil that reaches TWO nodes per side.
//
//   adv = (+0) + sum_a (u+ bq_a + u- fq_a) fl(1 / dx_a),  u+ = max(u, 0), u- = min(u, 0), u read at the node,
//   bq = 3/8 (x[+1] + x) - 7/8 x[-1] + 1/8 x[-2],   fq = 7/8 x[+1] - 3/8 (x[-1] + x) - 1/8 x[+2]
// every operation rounded on its own in the order of pa_device.h (pa_apply_terms, kind 5); on an axis without a periodic
// face the half whose far-upwind node would wrap -- bq at node index <= 1, fq at index >= N - 2 -- is the central
// difference 0.5 (x[+1] - x[-1]).  The Laplacian half and the STG combination are k_sf's, operation for operation.
//
// k_sf's design is kept: every WAVE marches along axis 0 on its own, RJ rows x 64 lanes x one 16-byte vector per lane, no
// LDS, no barrier, loads issued ahead of the arithmetic behind a sched_barrier, branch-free clamped plane pointers.  What
// the reach of 2 changes:
//   * planes: six register slots -- i-2 .. i+2 of the current plane and the one in flight (plane q + 3 is loaded while
//     plane q is computed) -- addressed by compile-time slot numbers: the plane loop is unrolled by six.
//   * rows: two halo rows above and two below the wave's row block, of the CURRENT plane only (loaded one plane ahead,
//     two slots); they wrap around inside the row axis like every roll stencil.
//   * along k: the second neighbour is the previous / next lane's component VEC-2+v / v (one more DPP move per row and
//     side), and every row has TWO edge cells per side of the tile: lane 0 keeps cells k0-1, k0-2, lane 63 k0+TK, k0+TK+1.
//   * fallback masks: per plane (uniform; the planes 0, 1, n0-2, n0-1 take the second copy of the body, like k_sf's planes
//     beside an axis-0 face), per row (uniform) and per lane component -- formed once in front of the loop.
//   * the planes -1 / -2 and n0 / n0+1 (clamped to the wrap planes glo / ghi): axis 0 is never periodic here
//     (pa_tile3d_step declines), so x[-2] at plane <= 1 and x[+2] at plane >= n0-2 only feed halves the fallback replaces;
//     x[-1] of plane 0 / x[+1] of plane n0-1 ARE read by the central fallback -- the wrap planes, as the generic kernel.
// US: sign of a SCALAR speed, known at launch -- 1: u >= 0 (bq only: planes i-2 .. i+1, rows j-2 .. j+1), 2: u < 0 (fq
// only).  The dead half is a signed zero that the accumulation absorbs: k_sf's argument (pa_sf_kernel.h "US") word for word,
// every field whose dead half (fq for u >= 0, bq for u < 0) is finite gives the bits of the generic kernel, which forms both
// halves; where it is inf or NaN the generic kernel has 0 x inf = NaN and this one a number.  The loads nobody uses (row j+2 / j-2,
// the far DPP move) fall away with it.  HASU: the speed is a field read at the node (US 0, both halves); a field that
// advects itself (u_field == phi) runs as HASU with the field as its own speed stream -- same bits, one more read stream
// that hits in cache.
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; VGPRs [+ AGPRs], the STG instantiation in brackets; no
// instantiation has a private segment):
//                    fp32 RJ 2    fp32 RJ 4               fp64 RJ 2    fp64 RJ 4
//   US 1 (u >= 0)    181 (185)    256 + 22 (256 + 26)     173 (181)    255 + 18 (255 + 34)
//   US 2 (u < 0)     175 (179)    256 +  8 (256 + 24)     169 (179)    255 + 14 (255 + 32)
//   HASU             213 (221)    256 + 68 (256 + 82)     211 (219)    256 + 76 (256 + 88)
// Two rows per wave: two waves per SIMD.  Four rows: the six plane slots alone are 96 VGPRs, the allocator fills the 256-VGPR
// file and parks values in AGPRs -- ONE wave per SIMD.  The rows-per-wave rule and what was measured: pa_sfq.hip, DESIGN.md
// section 4 "QUICK".
// SRC: the source term, k_sf's (pa_sf_kernel.h "SRC") word for word; instantiated for two rows per wave only (pa_sfq_src.hip).
// SCH: the scheme of the two halves, a trailing parameter whose default PA_OP_DIV_QUICK is every instantiation above.
// PA_OP_DIV_MINMOD / PA_OP_DIV_MC (pa_sft.hip; DESIGN.md section 4 "Bounded advection") take bq / fq from pa_tvd_halves
// (pa_device.h), component by component: the limited second-order halves, which read the same nodes i-2 .. i+2, and where
// QUICK falls back to central they fall back to first-order upwind, bq = x - x[-1] / fq = x[+1] - x -- so x[-1] of plane 0 /
// x[+1] of plane n0-1 are read there too (the wrap planes), and x[-2] / x[+2] beyond the ends again only feed halves the
// fallback replaces (dmm -> sm -> bq at plane <= 1, dpp -> sp -> fq at plane >= n0-2).  Nothing else depends on SCH: plane
// slots, halo rows, DPP moves, edge cells, the US dead half, the masks, the Laplacian half and STG are the code above.
// Registers of the SCH instantiations (two rows per wave, same source; no private segment, no AGPRs, two waves per SIMD):
//                    fp32 minmod   fp32 mc      fp64 minmod   fp64 mc
//   US 1 (u >= 0)    173 (179)     171 (178)    171 (179)     173 (181)
//   US 2 (u < 0)     173 (181)     173 (181)    171 (179)     173 (181)
//   HASU             205 (214)     211 (220)    213 (221)     215 (223)
#pragma once
#include "pa_sf_kernel.h"

template <typename T, int RJ, bool HASU, int US, bool STG, bool SRC = false, int SCH = PA_OP_DIV_QUICK>
__global__ void __launch_bounds__(256) k_sfq(Cg3dArgs<T> A) {
  static_assert(SCH == PA_OP_DIV_QUICK || SCH == PA_OP_DIV_MINMOD || SCH == PA_OP_DIV_MC, "SCH: a scheme with a reach of 2");
  static_assert(US == 0 || !HASU, "US: scalar speed");
  static_assert(HASU || US != 0, "a scalar speed has a sign");
  constexpr int VEC = VecOf<T>::N;
  typedef T V __attribute__((ext_vector_type(VEC)));
  constexpr int TJ = 4 * RJ, TK = 64 * VEC;
  constexpr bool BQ = US != 2, FQ = US != 1;   // the halves that are computed
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

  // ---- per-thread geometry: RJ rows x VEC columns, as 32-bit byte offsets inside a plane ------------
  const int kg = k0 + lane * VEC;
  const int kc = wrap(kg, n2);
  const bool kvalid = kg < n2;
  // lane 0: the two cells left of the tile, lane 63: the two right of it (e1 the nearer one)
  const int ecol1 = lane == 63 ? wrap(k0 + TK, n2) : wrap(k0 - 1, n2);
  const int ecol2 = lane == 63 ? wrap(k0 + TK + 1, n2) : wrap(k0 - 2, n2);
  const bool perJ = G.bct[2] == 4 || G.bct[3] == 4, perK = G.bct[4] == 4 || G.bct[5] == 4;
  unsigned off[RJ], offe1[RJ], offe2[RJ];
  bool rowOk[RJ], rLo[RJ], rHi[RJ];
  T cPj[RJ], cCj[RJ], cMj[RJ];     // Laplacian rows along j (uniform per row)
#pragma unroll
  for (int jj = 0; jj < RJ; ++jj) {
    const int jg = j0 + jj;
    const unsigned ro = (unsigned)wrap(jg, n1) * (unsigned)n2;
    off[jj] = (ro + (unsigned)kc) * (unsigned)sizeof(T);
    offe1[jj] = (ro + (unsigned)ecol1) * (unsigned)sizeof(T);
    offe2[jj] = (ro + (unsigned)ecol2) * (unsigned)sizeof(T);
    rowOk[jj] = kvalid && jg < n1;
    const int rc = pa_row_case(G, 1, jg, G.n1, G.treat);
    cPj[jj] = A.lap.inv[1]; cCj[jj] = A.lap.m2inv[1]; cMj[jj] = A.lap.inv[1];
    if (rc == 1) { cPj[jj] = A.lap.c23[1]; cCj[jj] = -A.lap.c23[1]; cMj[jj] = (T)0; }
    if (rc == 2) { cPj[jj] = (T)0; cCj[jj] = -A.lap.c23[1]; cMj[jj] = A.lap.c23[1]; }
    rLo[jj] = !perJ && jg <= 1;
    rHi[jj] = !perJ && jg >= n1 - 2;
  }
  // halo rows: [0] the nearer one (j0 - 1 / j0 + RJ), [1] the farther one (j0 - 2 / j0 + RJ + 1)
  unsigned offu[2], offd[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    offu[h] = ((unsigned)wrap(j0 - 1 - h, n1) * (unsigned)n2 + (unsigned)kc) * (unsigned)sizeof(T);
    offd[h] = ((unsigned)wrap(j0 + RJ + h, n1) * (unsigned)n2 + (unsigned)kc) * (unsigned)sizeof(T);
  }
  bool cLo[VEC], cHi[VEC];
  V cPkV, cCkV, cMkV;
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    const int kk = kg + v;
    const int rc = pa_row_case(G, 2, kk, G.n2, G.treat);
    T p = A.lap.inv[2], c0 = A.lap.m2inv[2], mq = A.lap.inv[2];
    if (rc == 1) { p = A.lap.c23[2]; c0 = -A.lap.c23[2]; mq = (T)0; }
    if (rc == 2) { p = (T)0; c0 = -A.lap.c23[2]; mq = A.lap.c23[2]; }
    cPkV[v] = p; cCkV[v] = c0; cMkV[v] = mq;
    cLo[v] = !perK && kk <= 1;
    cHi[v] = !perK && kk >= n2 - 2;
  }
  const size_t pstride = (size_t)G.s0 * sizeof(T);
  // uniform and BRANCH-FREE, every load unconditional on a clamped plane index (pa_sf_kernel.h `plane`)
  typedef const char __attribute__((address_space(1))) * gcptr;
  auto plane = [&](int ii) -> gcptr {
    const int ic = ii < 0 ? 0 : (ii >= n0 ? n0 - 1 : ii);
    uintptr_t u = (uintptr_t)A.d.p + (size_t)(unsigned)ic * pstride;
    const uintptr_t mlo = (uintptr_t)0 - (uintptr_t)(ii < 0), mhi = (uintptr_t)0 - (uintptr_t)(ii >= n0);
    u = (u & ~mlo) | ((uintptr_t)A.d.glo & mlo);
    u = (u & ~mhi) | ((uintptr_t)A.d.ghi & mhi);
    return (gcptr)u;
  };

  V uplC = (V)(T)0, umiC = (V)(T)0;   // scalar speed: u+ / u- once
  if (!HASU) {
    const T u = A.u;
    uplC = (V)(u < (T)0 ? (T)0 : u);
    umiC = (V)(u > (T)0 ? (T)0 : u);
  }

  // ---- register planes -----------------------------------------------------------------------------
  V P[6][RJ];              // own rows of six planes: slot of chunk-relative plane q is (q + 2) % 6
  V Hu[2][2], Hd[2][2];    // halo rows of the current plane: slot q & 1 (loaded one plane ahead)
  T He1[2][RJ], He2[2][RJ];   // edge cells of that plane
  V U[2][HASU ? RJ : 1];   // advection speed field of that plane

  auto load_own = [&](auto SLOT, int ii) {
    constexpr int s = decltype(SLOT)::value;
    gcptr p = plane(ii);
#pragma unroll
    for (int jj = 0; jj < RJ; ++jj) P[s][jj] = *reinterpret_cast<const V __attribute__((address_space(1)))*>(p + off[jj]);
  };
  auto load_halo = [&](auto SLOT, int ii) {   // ii inside the chunk
    constexpr int s = decltype(SLOT)::value;
    gcptr p = plane(ii);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      Hu[s][h] = *reinterpret_cast<const V __attribute__((address_space(1)))*>(p + offu[h]);
      Hd[s][h] = *reinterpret_cast<const V __attribute__((address_space(1)))*>(p + offd[h]);
    }
#pragma unroll
    for (int jj = 0; jj < RJ; ++jj) {
      He1[s][jj] = *reinterpret_cast<const T __attribute__((address_space(1)))*>(p + offe1[jj]);
      He2[s][jj] = *reinterpret_cast<const T __attribute__((address_space(1)))*>(p + offe2[jj]);
    }
    if constexpr (HASU) {
      const char* pu = (const char*)A.aux + (size_t)ii * pstride;
#pragma unroll
      for (int jj = 0; jj < RJ; ++jj) U[s][jj] = *reinterpret_cast<const V*>(pu + off[jj]);
    }
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  using I3 = std::integral_constant<int, 3>;
  using I4 = std::integral_constant<int, 4>;
  using I5 = std::integral_constant<int, 5>;

  // prologue: planes -2 .. 2 of the chunk (beyond it: the neighbour chunk's planes / the clamped wrap planes) and the
  // halo of plane 0
  load_own(I0{}, i0 - 2);
  load_own(I1{}, i0 - 1);
  load_own(I2{}, i0);
  load_halo(I0{}, i0);
  load_own(I3{}, i0 + 1);
  load_own(I4{}, i0 + 2);

  // one plane: C = q % 6 (q = chunk-relative plane index); slots i-2: C, i-1: C+1, current: C+2, i+1: C+3, i+2: C+4,
  // loading: C+5
  auto step = [&](auto CC, int q) {
    constexpr int C = decltype(CC)::value;
    constexpr int SMM = C % 6, SM = (C + 1) % 6, SC = (C + 2) % 6, SP = (C + 3) % 6, SPP = (C + 4) % 6, SL = (C + 5) % 6;
    constexpr int HC = C & 1, HN = (C + 1) & 1;
    const int ii = i0 + q;
    V Z[STG ? RJ : 1];   // STG: phi0 of THIS plane
    if constexpr (STG) {
      gcptr pz = (gcptr)((uintptr_t)A.stg_phi0 + (size_t)(unsigned)ii * pstride);
#pragma unroll
      for (int jj = 0; jj < RJ; ++jj) Z[jj] = *reinterpret_cast<const V __attribute__((address_space(1)))*>(pz + off[jj]);
    }
    V Sv[SRC ? RJ : 1];   // SRC: the source of THIS plane (pa_sf_kernel.h "SRC"; a scalar source reads the field's own rows)
    if constexpr (SRC) {
      gcptr ps = (gcptr)((uintptr_t)(A.src ? A.src : A.d.p) + (size_t)(unsigned)ii * pstride);
#pragma unroll
      for (int jj = 0; jj < RJ; ++jj) Sv[jj] = *reinterpret_cast<const V __attribute__((address_space(1)))*>(ps + off[jj]);
    }
    // loads for the next plane first: they fly during this plane's arithmetic
    load_own(std::integral_constant<int, SL>{}, ii + 3 <= i1 + 1 ? ii + 3 : i1 + 1);   // plane q + 3 (<= two behind the chunk)
    load_halo(std::integral_constant<int, HN>{}, ii + 1 < i1 ? ii + 1 : i1 - 1);
    __builtin_amdgcn_sched_barrier(0);   // keep them HERE (pa_sf_kernel.h)

    const int rci = pa_row_case(G, 0, (int64_t)ii, G.g0, G.treat);   // (no slab: off0 = 0, g0 = n0)
    const bool iLo_ = ii <= 1, iHi_ = ii >= n0 - 2;                   // axis 0 is not periodic here
    char* const po = (char*)A.out + (size_t)ii * pstride;
    auto body = [&](auto PLAINC) {
    constexpr bool PLAIN = decltype(PLAINC)::value;
    const bool iLo = PLAIN ? false : iLo_, iHi = PLAIN ? false : iHi_;
    T cPi = A.lap.inv[0], cCi = A.lap.m2inv[0], cMi = A.lap.inv[0];
    if (!PLAIN) {
      if (rci == 1) { cPi = A.lap.c23[0]; cCi = -A.lap.c23[0]; cMi = (T)0; }
      if (rci == 2) { cPi = (T)0; cCi = -A.lap.c23[0]; cMi = A.lap.c23[0]; }
    }
#pragma unroll
    for (int jj = 0; jj < RJ; ++jj) {
      const V xc = P[SC][jj];
      const V xpi = P[SP][jj], xmi = P[SM][jj], xppi = P[SPP][jj], xmmi = P[SMM][jj];
      // rows j-2 .. j+2 (after unrolling every index is a constant)
      V up, up2, dn, dn2;
      if (jj >= 1) up = P[SC][jj >= 1 ? jj - 1 : 0]; else up = Hu[HC][0];
      if (jj >= 2) up2 = P[SC][jj >= 2 ? jj - 2 : 0]; else up2 = Hu[HC][jj == 1 ? 0 : 1];
      if (jj + 1 < RJ) dn = P[SC][jj + 1 < RJ ? jj + 1 : 0]; else dn = Hd[HC][0];
      if (jj + 2 < RJ) dn2 = P[SC][jj + 2 < RJ ? jj + 2 : 0]; else dn2 = Hd[HC][jj + 2 - RJ > 0 ? 1 : 0];
      // k-2 .. k+2: inside the lane's vector, across lanes by DPP (lane 0 / 63 keep the tile's edge cells)
      V xpk, xmk, xppk, xmmk;
      const T e1 = He1[HC][jj], e2 = He2[HC][jj];
      const T pv1 = SfBits<T>::prev(xc[VEC - 1], e1);   // cell kg - 1
      const T nx1 = SfBits<T>::next(xc[0], e1);         // cell kg + VEC
      T pv2 = pv1, nx2 = nx1;
      if constexpr (BQ) pv2 = SfBits<T>::prev(xc[VEC - 2], e2);   // cell kg - 2
      if constexpr (FQ) nx2 = SfBits<T>::next(xc[1], e2);         // cell kg + VEC + 1
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        xpk[v] = (v + 1 < VEC) ? xc[v + 1 < VEC ? v + 1 : v] : nx1;
        xmk[v] = (v >= 1) ? xc[v >= 1 ? v - 1 : 0] : pv1;
        xppk[v] = (v + 2 < VEC) ? xc[v + 2 < VEC ? v + 2 : v] : (v + 2 == VEC ? nx1 : nx2);
        xmmk[v] = (v >= 2) ? xc[v >= 2 ? v - 2 : 0] : (v == 1 ? pv1 : pv2);
      }
      V axv;
      {   // the Laplacian: k_sf's row expressions
        V s = cPi * xpi;
        V mm = cCi * xc;
        s = s + mm;
        mm = cMi * xmi;
        s = s + mm;
        axv = s;
        s = cPj[jj] * dn;
        mm = cCj[jj] * xc;
        s = s + mm;
        mm = cMj[jj] * up;
        s = s + mm;
        axv = axv + s;
        s = cPkV * xpk;
        mm = cCkV * xc;
        s = s + mm;
        mm = cMkV * xmk;
        s = s + mm;
        axv = axv + s;
      }
      V upl = uplC, umi = umiC;
      if constexpr (HASU) {
        const V uc = U[HC][jj];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          upl[v] = uc[v] < (T)0 ? (T)0 : uc[v];
          umi[v] = uc[v] > (T)0 ? (T)0 : uc[v];
        }
      }
      V adv = (V)(T)0;
      // one axis: xp / xm / xpp / xmm its neighbours, lo / hi where bq / fq fall back (FB false: nowhere on this axis)
      auto axis = [&](auto FBC, const V& xp, const V& xm, const V& xpp, const V& xmm, auto lo, auto hi, T ih) {
        constexpr bool FB = decltype(FBC)::value;
        V cen = (V)(T)0;
        if constexpr (FB && SCH == PA_OP_DIV_QUICK) {
          cen = xp - xm;
          cen = (T)0.5 * cen;
        }
        V bq = (V)(T)0, fq = (V)(T)0;
        if constexpr (SCH != PA_OP_DIV_QUICK) {   // the limited halves (pa_device.h), first-order upwind where QUICK is central
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            bool l = false, h = false;
            if constexpr (FB) { l = lo(v); h = hi(v); }
            T b = (T)0, f = (T)0;
            pa_tvd_halves<T, BQ, FQ>(xmm[v], xm[v], xc[v], xp[v], xpp[v], l, h, SCH, b, f);
            bq[v] = b; fq[v] = f;
          }
        } else {
        if constexpr (BQ) {
          V t = xp + xc;
          t = (T)0.375 * t;
          V s = (T)0.875 * xm;
          t = t - s;
          s = (T)0.125 * xmm;
          bq = t + s;
          if constexpr (FB) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) bq[v] = lo(v) ? cen[v] : bq[v];
          }
        }
        if constexpr (FQ) {
          V t = xm + xc;
          t = (T)0.375 * t;
          V s = (T)0.875 * xp;
          t = s - t;
          s = (T)0.125 * xpp;
          fq = t - s;
          if constexpr (FB) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) fq[v] = hi(v) ? cen[v] : fq[v];
          }
        }
        }   // QUICK
        V t;
        if constexpr (US == 1) {          // u >= 0: u- = +0, its half is a signed zero
          t = upl * bq;
        } else if constexpr (US == 2) {   // u < 0: u+ = +0
          t = umi * fq;
        } else {
          t = upl * bq;
          V m2 = umi * fq;
          t = t + m2;
        }
        t = t * ih;
        adv = adv + t;
      };
      axis(std::integral_constant<bool, !PLAIN>{}, xpi, xmi, xppi, xmmi, [&](int) { return iLo; }, [&](int) { return iHi; }, A.ih[0]);
      axis(std::true_type{}, dn, up, dn2, up2, [&](int) { return rLo[jj]; }, [&](int) { return rHi[jj]; }, A.ih[1]);
      axis(std::true_type{}, xpk, xmk, xppk, xmmk, [&](int v) { return cLo[v]; }, [&](int v) { return cHi[v]; }, A.ih[2]);
      V qv = A.p0 * axv;
      qv = qv - adv;
      if constexpr (SRC) {   // a = a + s
        const bool hasF = A.src != nullptr;   // wave-uniform: a source field, else the splat of src_val
        V sv;
#pragma unroll
        for (int v = 0; v < VEC; ++v) sv[v] = hasF ? Sv[jj][v] : A.src_val;
        qv = qv + sv;
      }
      qv = A.p1 * qv;
      V res = xc + qv;
      if constexpr (STG) {
        V t0 = A.stg_c0 * Z[jj];
        V t1 = A.stg_c1 * res;
        res = t0 + t1;
      }
      if (rowOk[jj]) *reinterpret_cast<V*>(po + off[jj]) = res;
    }
    };   // body
    if (rci != 0 || iLo_ || iHi_) body(std::false_type{}); else body(std::true_type{});
  };

  for (int q = 0; q < CI; q += 6) {
    step(I0{}, q);
    if (q + 1 < CI) step(I1{}, q + 1);
    if (q + 2 < CI) step(I2{}, q + 2);
    if (q + 3 < CI) step(I3{}, q + 3);
    if (q + 4 < CI) step(I4{}, q + 4);
    if (q + 5 < CI) step(I5{}, q + 5);
  }
}

// ---- host side ---------------------------------------------------------------------------------------
template <typename T, int RJ, bool HASU, int US, bool STG, bool SRC = false, int SCH = PA_OP_DIV_QUICK>
static int launch_sfq(pa_ctx* c, Cg3dArgs<T>& A) {
  static int bpc = 0, dbg = -1;
  static const TileKernel K = {(const void*)k_sfq<T, RJ, HASU, US, STG, SRC, SCH>, RJ, VecOf<T>::N, 2, &bpc, &dbg,
    [](char* s, size_t n, const void* args) {
      const Cg3dArgs<T>& A = *(const Cg3dArgs<T>*)args;
      snprintf(s, n, "k_sfq phase 3 kind %d RJ %d%s%s%s%s", SCH, RJ, HASU ? " (speed field)" : (US == 1 ? " (u >= 0)" : " (u < 0)"), STG ? " (RK stage)" : "",
               A.aux && (const void*)A.aux == (const void*)A.d.p ? " (self)" : "", SRC ? " (source)" : "");
    }, false};
  return launch_tiled(c, K, c->G.n1, c->G.n2, &A, &A.tiles_j);
}

// V's instantiation of k_sfq for scheme SCH with / without SRC -- a speed field, or a scalar speed by its sign (US 1 / 2); plain
// and STG; one of the STATED row counts -- launched, or 0
template <typename T, bool SRC, int SCH, int... ROWS>
static int launch_sfq_speed(pa_ctx* c, Cg3dArgs<T>& A, const SfVariant& V) {
  return with_bool(V.stg, [&](auto stg) {
    return with_int<ROWS...>(V.rows, [&](auto rj) {
      constexpr bool STG = decltype(stg)::value;
      constexpr int RJ = decltype(rj)::value;
      if (V.hasu) return launch_sfq<T, RJ, true, 0, STG, SRC, SCH>(c, A);
      return with_int<1, 2>(V.us, [&](auto us) { return launch_sfq<T, RJ, false, decltype(us)::value, STG, SRC, SCH>(c, A); });
    });
  });
}
