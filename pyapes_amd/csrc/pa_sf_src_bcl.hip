// pa_sf_src_bcl.hip -- the SRC instantiations of k_sf (pa_sf_kernel.h) in the "BC on load" form: the upwind march with a
// source term and no BC-fill launch per step.  The source is read on the interior set only, so the form applies exactly
// where it does without a source (march_bcl_wanted, launch_sf_any).  Two or four rows per wave; scalar speed of either sign,
// speed field, SELF.  A translation unit of its own to keep the parallel build's slowest unit what it is.
#include "pa_sf_kernel.h"

template <typename T, bool HASU, int US, bool STG, bool SELF>
static int launch_sf_src_bcl_rows(pa_ctx* c, Cg3dArgs<T>& A, int rj) {
  return rj == 2 ? launch_sf<T, 2, 3, PA_OP_DIV_UPWIND, HASU, true, US, STG, SELF, true>(c, A)
                 : launch_sf<T, 4, 3, PA_OP_DIV_UPWIND, HASU, true, US, STG, SELF, true>(c, A);
}

template <typename T>
int pa_sf_euler_src_bcl(pa_ctx* c, Cg3dArgs<T>& A, int rj, bool stage, bool self) {
  if (rj != 2 && rj != 4) return 0;
  auto launch = [&](auto STGC) -> int {
    constexpr bool STG = decltype(STGC)::value;
    if (self) return launch_sf_src_bcl_rows<T, false, 0, STG, true>(c, A, rj);
    if (A.aux) return launch_sf_src_bcl_rows<T, true, 0, STG, false>(c, A, rj);
    if (A.u < (T)0) return launch_sf_src_bcl_rows<T, false, 2, STG, false>(c, A, rj);
    return launch_sf_src_bcl_rows<T, false, 1, STG, false>(c, A, rj);
  };
  return stage ? launch(std::true_type{}) : launch(std::false_type{});
}

template int pa_sf_euler_src_bcl<float>(pa_ctx*, Cg3dArgs<float>&, int, bool, bool);
template int pa_sf_euler_src_bcl<double>(pa_ctx*, Cg3dArgs<double>&, int, bool, bool);
