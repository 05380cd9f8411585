// pa_sf_vself.hip -- the VEL 3 instantiations of k_sf (pa_sf_kernel.h): the upwind explicit Euler step and the fused
// Runge-Kutta stage of ONE component of a vector field that advects itself (pa_momentum_march).  The velocity is the three
// components of the stage's input; the speed of the axis whose component is the target, A.vel_own, is the centre operand the row
// holds anyway, so two speed fields are read at the cell instead of three.  Two rows per wave, with and without a source term.
// Routing: pa_tile3d_euler_vel (pa_sf_vel.hip), the conditions of VEL 2.
#include "pa_sf_kernel.h"

template <typename T, bool STG>
static int launch_sf_vself(pa_ctx* c, Cg3dArgs<T>& A, bool source) {
  return source ? launch_sf<T, 2, 3, PA_OP_DIV_UPWIND, false, false, 0, STG, false, true, 3>(c, A)
                : launch_sf<T, 2, 3, PA_OP_DIV_UPWIND, false, false, 0, STG, false, false, 3>(c, A);
}

template <typename T>
int pa_sf_euler_vself(pa_ctx* c, Cg3dArgs<T>& A, bool stage, bool source) {
  return stage ? launch_sf_vself<T, true>(c, A, source) : launch_sf_vself<T, false>(c, A, source);
}

template int pa_sf_euler_vself<float>(pa_ctx*, Cg3dArgs<float>&, bool, bool);
template int pa_sf_euler_vself<double>(pa_ctx*, Cg3dArgs<double>&, bool, bool);
