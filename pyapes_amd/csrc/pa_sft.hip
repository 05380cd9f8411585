// pa_sft.hip -- the instantiations of k_sfq (pa_sfq_kernel.h) for the slope-limited schemes PA_OP_DIV_MINMOD / PA_OP_DIV_MC
// (template parameter SCH; DESIGN.md section 4 "Bounded advection"): the explicit Euler step / fused Runge-Kutta stage, two rows
// per wave, fp32 and fp64, US 1 / US 2 / HASU, plain and STG, for both limiters -- 24 kernels.  A translation unit of its own:
// the QUICK instantiations (pa_sfq.hip, pa_sfq_src.hip) are untouched.  pa_sfq_euler (pa_sfq.hip) calls in here; there are no
// SRC and no four-row instantiations (a source runs the generic kernel, option "sfq" = 4 means two rows).
#include "pa_sfq_kernel.h"

template <typename T, int SCH, bool STG>
static int launch_sft(pa_ctx* c, Cg3dArgs<T>& A) {
  if (A.aux) return launch_sfq<T, 2, true, 0, STG, false, SCH>(c, A);
  if (A.u < (T)0) return launch_sfq<T, 2, false, 2, STG, false, SCH>(c, A);
  return launch_sfq<T, 2, false, 1, STG, false, SCH>(c, A);
}

template <typename T>
int pa_sft_launch(pa_ctx* c, Cg3dArgs<T>& A, int kind, bool stage) {
  if (kind == PA_OP_DIV_MINMOD) return stage ? launch_sft<T, PA_OP_DIV_MINMOD, true>(c, A) : launch_sft<T, PA_OP_DIV_MINMOD, false>(c, A);
  if (kind == PA_OP_DIV_MC) return stage ? launch_sft<T, PA_OP_DIV_MC, true>(c, A) : launch_sft<T, PA_OP_DIV_MC, false>(c, A);
  return 0;
}

template int pa_sft_launch<float>(pa_ctx*, Cg3dArgs<float>&, int, bool);
template int pa_sft_launch<double>(pa_ctx*, Cg3dArgs<double>&, int, bool);
