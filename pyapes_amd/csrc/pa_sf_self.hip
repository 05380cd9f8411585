// pa_sf_self.hip -- the SELF instantiations of k_sf (pa_sf_kernel.h): the explicit Euler step and the fused Runge-Kutta
// stage of a field that advects itself, Div(phi, phi), for the three Div schemes; one, two or four rows per wave, BC on load
// (upwind) two or four.  A translation unit of its own because pa_sf.hip is already the slowest one of the parallel build.
#include "pa_sf_kernel.h"

template <typename T>
int pa_sf_launch_self(pa_ctx* c, Cg3dArgs<T>& A, const SfVariant& V) {
  if (!V.self || V.src || V.vel || V.hasu || V.us) return 0;
  return with_int<PA_OP_DIV_CENTRAL, PA_OP_DIV_UPWIND_COMPAT, PA_OP_DIV_UPWIND>(V.kind, [&](auto kind) {
    return with_bool(V.stg, [&](auto stg) {
      constexpr int KIND = decltype(kind)::value;
      constexpr bool STG = decltype(stg)::value;
      if constexpr (KIND == PA_OP_DIV_UPWIND) {
        if (V.bcl) return launch_sf_rows<T, 3, KIND, false, true, 0, STG, true, false, 0, 2, 4>(c, A, V);
      }
      return V.bcl ? 0 : launch_sf_rows<T, 3, KIND, false, false, 0, STG, true, false, 0, 1, 2, 4>(c, A, V);
    });
  });
}

template int pa_sf_launch_self<float>(pa_ctx*, Cg3dArgs<float>&, const SfVariant&);
template int pa_sf_launch_self<double>(pa_ctx*, Cg3dArgs<double>&, const SfVariant&);
