// pa_sfq_src.hip -- the SRC instantiations of k_sfq (pa_sfq_kernel.h): the QUICK Euler step / fused Runge-Kutta stage with
// a source term.  Two rows per wave only (the four-row kernels do not fit the register file, pa_sfq.hip): option "sfq" = 4
// with a source runs two rows.  pa_sfq_euler (pa_sfq.hip) calls in here.
#include "pa_sfq_kernel.h"

template <typename T>
int pa_sfq_launch_src(pa_ctx* c, Cg3dArgs<T>& A, bool stage) {
  auto launch = [&](auto STGC) -> int {
    constexpr bool STG = decltype(STGC)::value;
    if (A.aux) return launch_sfq<T, 2, true, 0, STG, true>(c, A);
    if (A.u < (T)0) return launch_sfq<T, 2, false, 2, STG, true>(c, A);
    return launch_sfq<T, 2, false, 1, STG, true>(c, A);
  };
  return stage ? launch(std::true_type{}) : launch(std::false_type{});
}

template int pa_sfq_launch_src<float>(pa_ctx*, Cg3dArgs<float>&, bool);
template int pa_sfq_launch_src<double>(pa_ctx*, Cg3dArgs<double>&, bool);
