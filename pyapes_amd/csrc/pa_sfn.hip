// pa_sfn.hip -- the instantiations of k_sfn (pa_sfn_kernel.h): the upwind Euler step / Runge-Kutta stage with a diffusivity
// field and one scalar speed, two rows per wave, fp32 and fp64.  A unit of its own, like the other variants of the step.
#include "pa_sfn_kernel.h"

template <typename T, int RJ, bool STG>
static int launch_sfn(pa_ctx* c, Cg3dArgs<T>& A) {
  static int bpc = 0, dbg = -1;
  static const TileKernel K = {(const void*)k_sfn<T, RJ, STG>, RJ, VecOf<T>::N, 2, &bpc, &dbg,
    [](char* s, size_t n, const void*) { snprintf(s, n, "k_sfn RJ %d%s (diffusivity field)", RJ, STG ? " (RK stage)" : ""); }, false};
  return launch_tiled(c, K, c->G.n1, c->G.n2, &A, &A.tiles_j);
}

template <typename T>
int pa_sfn_launch(pa_ctx* c, Cg3dArgs<T>& A, const SfVariant& V) {
  if (!V.nu || V.kind != PA_OP_DIV_UPWIND || V.hasu || V.self || V.src || V.vel || V.bcl || V.rows != 2) return 0;
  return with_bool(V.stg, [&](auto stg) { return launch_sfn<T, 2, decltype(stg)::value>(c, A); });
}

template int pa_sfn_launch<float>(pa_ctx*, Cg3dArgs<float>&, const SfVariant&);
template int pa_sfn_launch<double>(pa_ctx*, Cg3dArgs<double>&, const SfVariant&);
