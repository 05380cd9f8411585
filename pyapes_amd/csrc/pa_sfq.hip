// pa_sfq.hip -- the explicit Euler step / fused Runge-Kutta stage with the QUICK advection term on k_sfq
// (pa_sfq_kernel.h).  A translation unit of its own: k_sf and its instantiations (pa_sf.hip, pa_sf_self.hip) are untouched.
// step_t (pa_march.hip) asks here first for PA_OP_DIV_QUICK and for the limited kinds PA_OP_DIV_MINMOD / _MC (their
// instantiations: pa_sft.hip); 0 = not for k_sfq, the generic k_euler runs.
#include "pa_sfq_kernel.h"

// Rows per wave.  Four rows read (4 + 4) / 4 = 2 rows per row computed, two rows (2 + 4) / 2 = 3 -- the halo rows are the
// neighbour waves' own rows, cache hits.  But the four-row instantiations do not fit the 256-VGPR file (pa_sfq_kernel.h:
// 256 + 8 .. 88 AGPRs, ONE wave per SIMD, hundreds of v_accvgpr moves in the plane loop) where the two-row ones keep two
// waves per SIMD at 169 - 221 VGPRs: two rows everywhere.  The four-row kernels stay reachable through option "sfq" = 4
// for the A/B rows of bench_ops.py --sections quick (DESIGN.md section 4 "QUICK").  An axis has at least 5 nodes here, so
// there is no one-row form.
template <typename T>
static int sfq_rows_per_wave(pa_ctx* c) {
  return c->sfq == 4 ? 4 : 2;
}

template <typename T, bool STG>
static int launch_sfq_any(pa_ctx* c, Cg3dArgs<T>& A) {
  const bool four = sfq_rows_per_wave<T>(c) == 4;
  if (A.aux) return four ? launch_sfq<T, 4, true, 0, STG>(c, A) : launch_sfq<T, 2, true, 0, STG>(c, A);
  if (A.u < (T)0) return four ? launch_sfq<T, 4, false, 2, STG>(c, A) : launch_sfq<T, 2, false, 2, STG>(c, A);
  return four ? launch_sfq<T, 4, false, 1, STG>(c, A) : launch_sfq<T, 2, false, 1, STG>(c, A);
}

template <typename T>
int pa_sfq_euler(pa_ctx* c, Vec<T> phi, T* out, double u, const void* u_field, double nu, double dt, const T* phi0, double c0,
                 double c1, const pa_source* src, int kind) {
  const DevGeom& G = c->G;
  const bool limited = kind == PA_OP_DIV_MINMOD || kind == PA_OP_DIV_MC;
  if (kind != PA_OP_DIV_QUICK && !limited) return 0;
  if (limited && src) return 0;   // no SRC instantiations of the limited schemes (pa_sft.hip): the generic kernel
  if (!c->sfq || !c->sf || c->slab || c->ndim != 3 || !G.act[0] || G.n0 != G.g0 || G.off0 != 0) return 0;
  if (G.n0 < 5 || G.n1 < 5 || G.n2 < 5) return 0;
  if (G.bct[0] == PA_BC_PERIODIC || G.bct[1] == PA_BC_PERIODIC) return 0;   // the planes beyond the ends are not wrapped
  DevEq<T> E;
  pa_build_lap<T>(c, E);
  // whole 16-byte vectors, aligned operands (mode 1), option "fastpath"
  if (cg3d_mode<T>(c, E, {phi.p, out, u_field, phi.glo, phi.ghi, phi0, src ? src->field : nullptr}) != 1) return 0;
  Cg3dArgs<T> A;
  memset(&A, 0, sizeof(A));
  fill_common<T>(c, E, A);
  fill_h<T>(c, A);
  A.d = phi; A.out = out; A.aux = (const T*)u_field; A.u = (T)u; A.p0 = (T)nu; A.p1 = (T)dt; A.kind = kind;
  A.stg_phi0 = phi0; A.stg_c0 = (T)c0; A.stg_c1 = (T)c1;
  {  // k_sfq writes the step's value at EVERY node: only where the BC fill behind it rewrites all nodes outside the interior set
    int faces = 0;
    for (int f = 0; f < 6; ++f) faces += (G.act[f >> 1] && c->bc[f].type != PA_BC_NONE) ? 1 : 0;
    A.out_all = faces == 6 ? 1 : 0;
  }
  if (!sf_applies<T, 3>(c, A, 1)) return 0;
  int n;
  if (limited) {   // pa_sft.hip: two rows per wave, whatever option "sfq" says
    n = pa_sft_launch<T>(c, A, kind, phi0 != nullptr);
  } else if (src) {   // the SRC instantiations (pa_sfq_src.hip): two rows per wave, whatever option "sfq" says
    A.src = (const T*)src->field; A.src_val = (T)src->value;
    n = pa_sfq_launch_src<T>(c, A, phi0 != nullptr);
  } else {
    n = phi0 ? launch_sfq_any<T, true>(c, A) : launch_sfq_any<T, false>(c, A);
  }
  if (n > 0 && hipGetLastError() != hipSuccess) { pa_set_err(c, "k_sfq launch failed"); return PA_E_HIP; }
  return n;
}

template int pa_sfq_euler<float>(pa_ctx*, Vec<float>, float*, double, const void*, double, double, const float*, double, double, const pa_source*, int);
template int pa_sfq_euler<double>(pa_ctx*, Vec<double>, double*, double, const void*, double, double, const double*, double, double, const pa_source*, int);
