// pa_stats.hip -- the flow diagnostics of a time loop (DESIGN.md section 4 "Flow diagnostics"): pa_flow_stats, four numbers
// of the BC-filled vector field U in ONE pass over its d components -- what a user needs to choose dt (the CFL rate), to judge
// a projection (the divergence it left, as a maximum and as a sum of squares) and to watch the run (the kinetic energy).
//
// The arithmetic is a definition of this library.  Per node, every operation rounded on its own in the grid dtype (no FMA),
// q_a = 1 / dx_a and h_a = 0.5 / dx_a formed in double on the host and converted once, axes ascending:
//   rate      max over ALL nodes of s:          r = |U_a| * q_a;  s = s + r                      (s starts at +0)
//   div_max   max over the interior set of |s|: d = U_a[+1]_a - U_a[-1]_a;  d = d * h_a;  s = s + d   (proj_div_sum)
//   div_sq    sum over the interior set of (double)(s * s), that s
//   ke_sq     sum over all nodes and axes of (double)(U_a * U_a)
// The maxima are carried as doubles (an exact conversion) and a NaN in any contribution makes that maximum NaN (pa_max_nan);
// the sums are accumulated in double in the order the grid gives them.
//
// Stage one: one cell per lane in a grid-stride loop under PA_MAX_GRID, every block leaving two sums and two maxima in the
// context's scratch; stage two: one block folds the rows, in a fixed order.  One copy of the four doubles, one synchronise.
#include "pa_project.h"

template <typename T>
struct StatInv { T q[3]; };   // q[a] = (T)(1 / dx_a), internal axes

__device__ __forceinline__ float pa_abs(float x) { return __builtin_fabsf(x); }
__device__ __forceinline__ double pa_abs(double x) { return __builtin_fabs(x); }

// partials: gridDim.x rows of (div_sq, ke_sq), then gridDim.x rows of (rate, div_max)
template <typename T>
__global__ void __launch_bounds__(PA_BLOCK) k_flow_stats(DevGeom G, ProjVec<T> U, StatInv<T> Q, double* __restrict__ partials) {
  double sum[2] = {0.0, 0.0};
  double mx[2] = {0.0, 0.0};
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < G.ncell;
       idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t i, j, k;
    pa_decode(G, idx, i, j, k);
    T s = (T)0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (!G.act[a]) continue;
      const T u = U.v[a].p[idx];
      T r = pa_abs(u) * Q.q[a];
      s = s + r;
      T e = u * u;
      sum[1] += (double)e;
    }
    mx[0] = pa_max_nan(mx[0], (double)s);
    if (pa_in_S(G, i, j, k)) {
      const T d = proj_div_sum<T>(G, U, i, j, k);
      mx[1] = pa_max_nan(mx[1], (double)pa_abs(d));
      T e = d * d;
      sum[0] += (double)e;
    }
  }
  pa_block_reduce_store<2>(sum, partials);
  pa_block_reduce_max_store<2>(mx, partials + 2 * (int64_t)gridDim.x);
}

// out: rate, div_max, div_sq, ke_sq
__global__ void __launch_bounds__(PA_BLOCK) k_flow_stats_final(const double* __restrict__ partials, int nblk, double* __restrict__ out) {
  double sum[2] = {0.0, 0.0};
  double mx[2] = {0.0, 0.0};
  for (int b = threadIdx.x; b < nblk; b += blockDim.x) {
    sum[0] += partials[2 * b];
    sum[1] += partials[2 * b + 1];
    mx[0] = pa_max_nan(mx[0], partials[2 * (nblk + b)]);
    mx[1] = pa_max_nan(mx[1], partials[2 * (nblk + b) + 1]);
  }
  pa_block_reduce_max_store<2>(mx, out);
  pa_block_reduce_store<2>(sum, out + 2);
}

template <typename T>
static int stats_t(pa_ctx* c, const void* U, double* result) {
  static int dbg = -1;
  if (proj_dbg(&dbg, 64)) fprintf(stderr, "[pyapes_hip] k_flow_stats: generic kernel, %lld cells\n", (long long)c->G.ncell);
  int rc;
  if ((rc = pa_scratch(c, &c->scr[SCR_STATS], &c->cap[SCR_STATS], (size_t)(4 * PA_MAX_GRID + 4) * sizeof(double)))) return rc;
  double* part = (double*)c->scr[SCR_STATS];
  double* out = part + 4 * PA_MAX_GRID;
  const int nb = pa_grid_blocks(c->G.ncell);
  StatInv<T> Q;
  for (int a = 0; a < 3; ++a) Q.q[a] = (T)(1.0 / c->dx[a]);
  hipLaunchKernelGGL(k_flow_stats<T>, dim3(nb), dim3(PA_BLOCK), 0, c->stream, c->G, proj_vec<T>(c, U), Q, part);
  hipLaunchKernelGGL(k_flow_stats_final, dim3(1), dim3(PA_BLOCK), 0, c->stream, (const double*)part, nb, out);
  PA_HIP(c, hipGetLastError());
  PA_HIP(c, hipMemcpyAsync(result, out, 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  PA_HIP(c, hipStreamSynchronize(c->stream));
  return PA_OK;
}

extern "C" {

int pa_flow_stats(pa_ctx* c, const void* U, int ncomp, double* result) {
  const char* who = "pa_flow_stats";
  if (int rc = check_projection_call(c, who, ncomp)) return rc;
  if (!U || !result) { pa_set_err(c, "%s: U and result are needed", who); return PA_E_ARG; }
  PaRange range_("pyapes flow statistics");
  PA_HIP(c, hipSetDevice(c->device));
  return c->dtype == PA_F64 ? stats_t<double>(c, U, result) : stats_t<float>(c, U, result);
}

}  // extern "C"
