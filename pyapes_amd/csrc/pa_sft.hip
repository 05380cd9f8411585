// pa_sft.hip -- the instantiations of k_sfq (pa_sfq_kernel.h) for the slope-limited schemes PA_OP_DIV_MINMOD / PA_OP_DIV_MC
// (template parameter SCH; DESIGN.md section 4 "Bounded advection"): the explicit Euler step / fused Runge-Kutta stage, two rows
// per wave, fp32 and fp64, US 1 / US 2 / HASU, plain and STG, for both limiters -- 24 kernels.  A translation unit of its own:
// the QUICK instantiations (pa_sfq.hip, pa_sfq_src.hip) are untouched.  There are no SRC and no four-row instantiations (a
// source runs the generic kernel, option "sfq" = 4 means two rows).
#include "pa_sfq_kernel.h"

template <typename T>
int pa_sft_launch(pa_ctx* c, Cg3dArgs<T>& A, const SfVariant& V) {
  if (V.src) return 0;
  return with_int<PA_OP_DIV_MINMOD, PA_OP_DIV_MC>(V.kind, [&](auto sch) { return launch_sfq_speed<T, false, decltype(sch)::value, 2>(c, A, V); });
}

template int pa_sft_launch<float>(pa_ctx*, Cg3dArgs<float>&, const SfVariant&);
template int pa_sft_launch<double>(pa_ctx*, Cg3dArgs<double>&, const SfVariant&);
