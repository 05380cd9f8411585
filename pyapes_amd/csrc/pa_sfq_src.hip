// pa_sfq_src.hip -- the SRC instantiations of k_sfq (pa_sfq_kernel.h): the QUICK Euler step / fused Runge-Kutta stage with
// a source term.  Two rows per wave only (the four-row kernels do not fit the register file, sf_variant): option "sfq" = 4
// with a source runs two rows.
#include "pa_sfq_kernel.h"

template <typename T>
int pa_sfq_launch_src(pa_ctx* c, Cg3dArgs<T>& A, const SfVariant& V) {
  if (V.kind != PA_OP_DIV_QUICK || !V.src) return 0;
  return launch_sfq_speed<T, true, PA_OP_DIV_QUICK, 2>(c, A, V);
}

template int pa_sfq_launch_src<float>(pa_ctx*, Cg3dArgs<float>&, const SfVariant&);
template int pa_sfq_launch_src<double>(pa_ctx*, Cg3dArgs<double>&, const SfVariant&);
