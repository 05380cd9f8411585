// pa_sf_vself.hip -- the VEL 3 instantiations of k_sf (pa_sf_kernel.h): the upwind explicit Euler step and the fused
// Runge-Kutta stage of ONE component of a vector field that advects itself (pa_momentum_march).  The velocity is the three
// components of the stage's input; the speed of the axis whose component is the target, A.vel_own, is the centre operand the row
// holds anyway, so two speed fields are read at the cell instead of three.  Two rows per wave, with and without a source term.
// The conditions are those of VEL 2 (pa_tile3d_step, pa_sf.hip); sf_variant (pa_sf_kernel.h) tells the two apart.
#include "pa_sf_kernel.h"

template <typename T>
int pa_sf_launch_vself(pa_ctx* c, Cg3dArgs<T>& A, const SfVariant& V) {
  if (V.vel != 3 || V.kind != PA_OP_DIV_UPWIND || V.hasu || V.bcl || V.us || V.self) return 0;
  return with_bool(V.stg, [&](auto stg) {
    return with_bool(V.src, [&](auto src) {
      return launch_sf_rows<T, 3, PA_OP_DIV_UPWIND, false, false, 0, decltype(stg)::value, false, decltype(src)::value, 3, 2>(c, A, V);
    });
  });
}

template int pa_sf_launch_vself<float>(pa_ctx*, Cg3dArgs<float>&, const SfVariant&);
template int pa_sf_launch_vself<double>(pa_ctx*, Cg3dArgs<double>&, const SfVariant&);
