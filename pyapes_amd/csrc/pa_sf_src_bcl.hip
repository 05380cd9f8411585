// pa_sf_src_bcl.hip -- the SRC instantiations of k_sf (pa_sf_kernel.h) in the "BC on load" form: the upwind march with a
// source term and no BC-fill launch per step.  The source is read on the interior set only, so the form applies exactly
// where it does without a source (march_bcl_wanted, sf_variant).  Two or four rows per wave (the fp64 stage with a speed field: two); scalar speed of either sign,
// speed field, SELF.  A translation unit of its own to keep the parallel build's slowest unit what it is.
#include "pa_sf_kernel.h"

template <typename T, bool HASU, int US, bool STG, bool SELF>
static int launch_sf_src_bcl_rows(pa_ctx* c, Cg3dArgs<T>& A, const SfVariant& V) {
  // (fp64, a speed field, the stage: two rows only -- sf_variant never asks for four)
  if constexpr (sizeof(T) == 8 && HASU && STG) return launch_sf_rows<T, 3, PA_OP_DIV_UPWIND, HASU, true, US, STG, SELF, true, 0, 2>(c, A, V);
  else return launch_sf_rows<T, 3, PA_OP_DIV_UPWIND, HASU, true, US, STG, SELF, true, 0, 2, 4>(c, A, V);
}

template <typename T>
int pa_sf_launch_src_bcl(pa_ctx* c, Cg3dArgs<T>& A, const SfVariant& V) {
  if (!V.src || !V.bcl || V.vel || V.kind != PA_OP_DIV_UPWIND) return 0;
  return with_bool(V.stg, [&](auto stg) {
    constexpr bool STG = decltype(stg)::value;
    if (V.self) return launch_sf_src_bcl_rows<T, false, 0, STG, true>(c, A, V);
    if (V.hasu) return launch_sf_src_bcl_rows<T, true, 0, STG, false>(c, A, V);
    return with_int<1, 2>(V.us, [&](auto us) { return launch_sf_src_bcl_rows<T, false, decltype(us)::value, STG, false>(c, A, V); });
  });
}

template int pa_sf_launch_src_bcl<float>(pa_ctx*, Cg3dArgs<float>&, const SfVariant&);
template int pa_sf_launch_src_bcl<double>(pa_ctx*, Cg3dArgs<double>&, const SfVariant&);
