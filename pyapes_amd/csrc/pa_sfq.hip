// pa_sfq.hip -- the instantiations of k_sfq (pa_sfq_kernel.h) for the QUICK advection term without a source: the explicit
// Euler step / fused Runge-Kutta stage, two rows per wave and -- option "sfq" = 4 -- four, a scalar speed of either sign or a
// speed field.  A translation unit of its own: k_sf and its instantiations are untouched.  pa_tile3d_step (pa_sf.hip) routes
// PA_OP_DIV_QUICK and the limited kinds PA_OP_DIV_MINMOD / _MC (pa_sft.hip) to k_sfq or to nothing: the generic k_euler runs.
#include "pa_sfq_kernel.h"

template <typename T>
int pa_sfq_launch(pa_ctx* c, Cg3dArgs<T>& A, const SfVariant& V) {
  if (V.kind != PA_OP_DIV_QUICK || V.src) return 0;
  return launch_sfq_speed<T, false, PA_OP_DIV_QUICK, 2, 4>(c, A, V);
}

template int pa_sfq_launch<float>(pa_ctx*, Cg3dArgs<float>&, const SfVariant&);
template int pa_sfq_launch<double>(pa_ctx*, Cg3dArgs<double>&, const SfVariant&);
