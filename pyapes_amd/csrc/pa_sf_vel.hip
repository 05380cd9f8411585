// pa_sf_vel.hip -- the VEL instantiations of k_sf (pa_sf_kernel.h): the upwind explicit Euler step and the fused Runge-Kutta
// stage in a velocity field, one advection speed per mesh axis (pa_*_vel).  Three scalar speeds (VEL 1) or three speed fields
// read at the cell (VEL 2), two rows per wave, with and without a source term.  Everything else with a velocity -- central,
// QUICK, 1-D / 2-D meshes, odd rows, unaligned operands, a periodic axis 0, a mix of scalar and field components, n1 <= 4 --
// runs the generic k_euler (pa_march.hip): pa_tile3d_step (pa_sf.hip) returns 0 for it.  A target that is itself one of the three
// speed fields (pa_momentum_march, own >= 0) takes the VEL 3 instantiations of pa_sf_vself.hip under the same conditions.
#include "pa_sf_kernel.h"

template <typename T>
int pa_sf_launch_vel(pa_ctx* c, Cg3dArgs<T>& A, const SfVariant& V) {
  if (V.kind != PA_OP_DIV_UPWIND || V.hasu || V.bcl || V.us || V.self) return 0;
  return with_int<1, 2>(V.vel, [&](auto vel) {
    return with_bool(V.stg, [&](auto stg) {
      return with_bool(V.src, [&](auto src) {
        return launch_sf_rows<T, 3, PA_OP_DIV_UPWIND, false, false, 0, decltype(stg)::value, false, decltype(src)::value, decltype(vel)::value, 2>(c, A, V);
      });
    });
  });
}

template int pa_sf_launch_vel<float>(pa_ctx*, Cg3dArgs<float>&, const SfVariant&);
template int pa_sf_launch_vel<double>(pa_ctx*, Cg3dArgs<double>&, const SfVariant&);
