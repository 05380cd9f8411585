// pa_sf_src.hip -- the SRC instantiations of k_sf (pa_sf_kernel.h): the explicit Euler step and the fused Runge-Kutta stage
// with a source term, d(phi)/dt = nu lap(phi) - div(u phi) + S.  Upwind with a scalar speed of either sign (US 1 / 2), a speed
// field, or the field itself (SELF); central with a scalar speed or SELF; one, two or four rows per wave.  The BC-on-load
// forms are in pa_sf_src_bcl.hip; the literal upwind form has none (generic kernel).  pa_tile3d_euler (pa_sf.hip) calls in
// here.
#include "pa_sf_kernel.h"

template <typename T, int KIND, bool HASU, int US, bool STG, bool SELF>
static int launch_sf_src_rows(pa_ctx* c, Cg3dArgs<T>& A) {
  switch (sf_rows_per_wave<T>(c)) {
    case 1: return launch_sf<T, 1, 3, KIND, HASU, false, US, STG, SELF, true>(c, A);
    case 2: return launch_sf<T, 2, 3, KIND, HASU, false, US, STG, SELF, true>(c, A);
    default: return launch_sf<T, 4, 3, KIND, HASU, false, US, STG, SELF, true>(c, A);
  }
}

template <typename T>
int pa_sf_euler_src(pa_ctx* c, Cg3dArgs<T>& A, int kind, bool stage, bool self) {
  auto launch = [&](auto STGC) -> int {
    constexpr bool STG = decltype(STGC)::value;
    if (kind == PA_OP_DIV_UPWIND) {
      if (self) return launch_sf_src_rows<T, PA_OP_DIV_UPWIND, false, 0, STG, true>(c, A);
      if (A.aux) return launch_sf_src_rows<T, PA_OP_DIV_UPWIND, true, 0, STG, false>(c, A);
      if (A.u < (T)0) return launch_sf_src_rows<T, PA_OP_DIV_UPWIND, false, 2, STG, false>(c, A);
      return launch_sf_src_rows<T, PA_OP_DIV_UPWIND, false, 1, STG, false>(c, A);
    }
    if (kind == PA_OP_DIV_CENTRAL) {
      if (self) return launch_sf_src_rows<T, PA_OP_DIV_CENTRAL, false, 0, STG, true>(c, A);
      if (A.aux) return 0;   // a foreign speed field: generic kernel (pa_tile3d_euler declines it before it gets here)
      return launch_sf_src_rows<T, PA_OP_DIV_CENTRAL, false, 0, STG, false>(c, A);
    }
    return 0;
  };
  return stage ? launch(std::true_type{}) : launch(std::false_type{});
}

template int pa_sf_euler_src<float>(pa_ctx*, Cg3dArgs<float>&, int, bool, bool);
template int pa_sf_euler_src<double>(pa_ctx*, Cg3dArgs<double>&, int, bool, bool);
