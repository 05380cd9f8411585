// pa_solver.h -- what the solver translation units share: pa_solver.hip (the kernels two methods launch, the host
// helpers of every driver), pa_cg.hip, pa_bicgstab.hip, pa_jacobi.hip.  A kernel has exactly one home; the other
// units reach it through the launchers below (explicitly instantiated for float / double in pa_solver.hip).
#pragma once
#include "pa_host.h"
#include "pa_scalar_steps.h"

#include <math.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <new>

// ---- reductions of per-block partials + scalar logic ------------------------------------
// sums[slot[s]] (+)= sum over blocks of partials[b*ns + s]
__device__ __forceinline__ double pa_reduce_partials(const double* __restrict__ partials, int nblk, int ns,
                                                     int s, double* sm) {
  double v = 0.0;
  for (int b = threadIdx.x; b < nblk; b += blockDim.x) v += partials[(int64_t)b * ns + s];
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += sm[w];
  __syncthreads();
  return t;  // valid on thread 0
}

// ---- host side (pa_solver.hip) ------------------------------------------------------------
int init_scalars(pa_ctx* c, double tol, int64_t max_it);
int read_scalars(pa_ctx* c);

// Pipelined poll: after a batch of iterations, queue a copy of the device scalars and wait for the copy of the PREVIOUS
// batch, so the GPU always has a batch queued (one after the done flag is set is no-ops: every kernel starts with
// `if (done) return`).  A synchronous poll idles the GPU ~250 us per ~300 us of work on the reference's meshes.
struct PollPipe {
  int pending = -1, slot = 0;
};
int poll_submit(pa_ctx* c, PollPipe& P, bool* done);
int poll_drain(pa_ctx* c, PollPipe& P, bool* done);
int poll_interval(const pa_ctx* c);   // iterations per batch between host polls of the done flag

// One-shot drivers.  try_resident: small meshes, the whole solve in one cooperative launch (pa_resident.hip; kind 0 CG,
// 1 Jacobi, 2 BiCGSTAB).  1: that launch ended the solve (*rc: the status), 0: the caller runs its launch-per-phase loop
// (not covered, or a bounded grid-wide wait gave up and left x, r and the scalars untouched).  Records ev0 either way.
template <typename T>
int try_resident(pa_ctx* c, int kind, T* x, const T* rhs, double tol, int64_t max_it, double omega, pa_report* out,
                 int* rc);
// the timed tail of a one-shot solve whose scalars have been read back: ev1, elapsed time since ev0, the report
int timed_report(pa_ctx* c, pa_report* out);

// r = (b - A x) on S (0 elsewhere), d = r, per-block partial sums of r.r: the tiled A x kernel plus one
// streaming pass where the tiled kernel applies, else the generic kernel
template <typename T>
int cg_residual_init(pa_ctx* c, const DevEq<T>& E, Vec<T> xv, const T* rhs, T* r, T* d, T* send_lo, T* send_hi,
                     double* part);
// the same into the PITCH layout (c->cg_ps1), A x through the contiguous scratch `ax`; where the tiled A x declines
// (not rz) nothing is launched and the solve goes back to the contiguous layout (c->cg_pitch = 0)
template <typename T>
int cg_residual_init_pitch(pa_ctx* c, const DevEq<T>& E, Vec<T> xv, const T* rhs, T* ax, T* r, T* d, double* part);
template <typename T>
int64_t solver_pitch(const pa_ctx* c, const T* x);
// a field of the slab solver with its ghost planes; a physical (non-periodic) end has none: no result uses that plane
// (the end plane is a boundary node), the field's own end plane stands in so that speculative loads stay in valid memory
template <typename T>
Vec<T> slab_vec(const pa_ctx* c, const T* p, const void* glo, const void* ghi);

// launchers of the kernels the methods share
template <typename T>
void launch_post_init(pa_ctx* c, const double* part, int nblk, int stage);   // k_cg_post_init -> sums[1], rr
template <typename T>
void copy_x_old(pa_ctx* c, const T* x);        // x -> x_old_out (pa_solver_keep_old) unless the solve is over
template <typename T>
void pack_x_planes(pa_ctx* c, const T* x);     // periodic ring ends: x[1] / x[n0-1] / x[n0-2] -> x_pack_*
template <typename T>
void pack_end_planes(pa_ctx* c, const T* a, void* lo, void* hi);   // first / last owned plane of a -> lo / hi
