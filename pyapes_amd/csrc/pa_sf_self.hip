// pa_sf_self.hip -- the SELF instantiations of k_sf (pa_sf_kernel.h): the explicit Euler step and the fused Runge-Kutta
// stage of a field that advects itself, Div(phi, phi), for the three Div schemes.  A translation unit of its own because
// pa_sf.hip is already the slowest one of the parallel build; pa_tile3d_euler (pa_sf.hip) calls in here.
#include "pa_sf_kernel.h"

template <typename T>
int pa_sf_euler_self(pa_ctx* c, Cg3dArgs<T>& A, int kind, bool stage) {
  auto launch = [&](auto STGC) -> int {
    constexpr bool STG = decltype(STGC)::value;
    switch (kind) {
      case PA_OP_DIV_CENTRAL: return launch_sf_self<T, PA_OP_DIV_CENTRAL, STG>(c, A);
      case PA_OP_DIV_UPWIND_COMPAT: return launch_sf_self<T, PA_OP_DIV_UPWIND_COMPAT, STG>(c, A);
      case PA_OP_DIV_UPWIND: return launch_sf_self<T, PA_OP_DIV_UPWIND, STG>(c, A);
      default: return 0;
    }
  };
  return stage ? launch(std::true_type{}) : launch(std::false_type{});
}

template int pa_sf_euler_self<float>(pa_ctx*, Cg3dArgs<float>&, int, bool);
template int pa_sf_euler_self<double>(pa_ctx*, Cg3dArgs<double>&, int, bool);
