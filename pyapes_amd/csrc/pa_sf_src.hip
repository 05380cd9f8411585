// pa_sf_src.hip -- the SRC instantiations of k_sf (pa_sf_kernel.h): the explicit Euler step and the fused Runge-Kutta stage
// with a source term, d(phi)/dt = nu lap(phi) - div(u phi) + S.  Upwind with a scalar speed of either sign (US 1 / 2), a speed
// field, or the field itself (SELF); central with a scalar speed or SELF; one, two or four rows per wave.  The BC-on-load
// forms are in pa_sf_src_bcl.hip; the literal upwind form has none (generic kernel).
#include "pa_sf_kernel.h"

template <typename T, int KIND, bool HASU, int US, bool STG, bool SELF>
static int launch_sf_src_rows(pa_ctx* c, Cg3dArgs<T>& A, const SfVariant& V) {
  return launch_sf_rows<T, 3, KIND, HASU, false, US, STG, SELF, true, 0, 1, 2, 4>(c, A, V);
}

template <typename T>
int pa_sf_launch_src(pa_ctx* c, Cg3dArgs<T>& A, const SfVariant& V) {
  if (!V.src || V.bcl || V.vel) return 0;
  return with_bool(V.stg, [&](auto stg) {
    constexpr bool STG = decltype(stg)::value;
    if (V.kind == PA_OP_DIV_UPWIND) {
      if (V.self) return launch_sf_src_rows<T, PA_OP_DIV_UPWIND, false, 0, STG, true>(c, A, V);
      if (V.hasu) return launch_sf_src_rows<T, PA_OP_DIV_UPWIND, true, 0, STG, false>(c, A, V);
      return with_int<1, 2>(V.us, [&](auto us) { return launch_sf_src_rows<T, PA_OP_DIV_UPWIND, false, decltype(us)::value, STG, false>(c, A, V); });
    }
    if (V.kind == PA_OP_DIV_CENTRAL) {
      if (V.self) return launch_sf_src_rows<T, PA_OP_DIV_CENTRAL, false, 0, STG, true>(c, A, V);
      if (V.hasu) return 0;   // a foreign speed field: generic kernel (pa_tile3d_step declines it before it gets here)
      return launch_sf_src_rows<T, PA_OP_DIV_CENTRAL, false, 0, STG, false>(c, A, V);
    }
    return 0;
  });
}

template int pa_sf_launch_src<float>(pa_ctx*, Cg3dArgs<float>&, const SfVariant&);
template int pa_sf_launch_src<double>(pa_ctx*, Cg3dArgs<double>&, const SfVariant&);
