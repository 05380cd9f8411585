// pa_project.h -- what the translation units of the projection layer share (pa_project.hip, pa_stats.hip): the vector operand
// of a one-pass kernel over the components, the two per-cell arithmetic statements (the divergence sum, the corrected value
// of a component), the launch-log budget, and the refusals made before anything is enqueued.
#pragma once
#include "pa_host.h"

#include <stdlib.h>
#include <stdio.h>

#include <initializer_list>

// one pointer per INTERNAL axis (a d-dimensional mesh occupies the last d), the ghost planes being the field's own wrap-around
// planes; h[a] = (T)(0.5 / dx_a)
template <typename T>
struct ProjVec {
  Vec<T> v[3];
  T h[3];
};

// PYAPES_HIP_DEBUG: one line per launch, `budget` of them per print site
static inline bool proj_dbg(int* left, int budget) {
  if (*left < 0) *left = getenv("PYAPES_HIP_DEBUG") ? budget : 0;
  if (*left <= 0) return false;
  --*left;
  return true;
}

template <typename T>
static inline ProjVec<T> proj_vec(const pa_ctx* c, const void* U) {
  ProjVec<T> P;
  const int sh = 3 - c->ndim;
  for (int a = 0; a < 3; ++a) {
    const T* comp = (const T*)U + (int64_t)(a >= sh ? a - sh : 0) * c->G.ncell;   // (an inactive axis: never read)
    P.v[a] = pa_vec_self<T>(c, comp);
    P.h[a] = (T)(0.5 / c->dx[a]);
  }
  return P;
}

// where component a of a correction goes (o[a] == U.v[a].p: in place -- a cell's value is read and written by the same lane,
// and no lane reads another cell of U)
template <typename T>
struct ProjOut { T* o[3]; };

template <typename T>
static inline ProjOut<T> proj_out(const pa_ctx* c, void* out) {
  ProjOut<T> O;
  const int sh = 3 - c->ndim;
  for (int a = 0; a < 3; ++a) O.o[a] = (T*)out + (int64_t)(a >= sh ? a - sh : 0) * c->G.ncell;
  return O;
}

// the divergence sum of cell (i, j, k) of the interior set:  d = U_a[+1]_a - U_a[-1]_a;  d = d * h_a;  s = s + d, s from +0,
// axes ascending, every operation rounded on its own
template <typename T>
__device__ __forceinline__ T proj_div_sum(const DevGeom& G, const ProjVec<T>& U, int64_t i, int64_t j, int64_t k) {
  T s = (T)0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!G.act[a]) continue;
    FieldAcc<T> acc{U.v[a]};
    T xp, xm;
    pa_nbrs<T>(G, acc, a, i, j, k, xp, xm);
    T d = xp - xm;
    d = d * U.h[a];
    s = s + d;
  }
  return s;
}

// component a at cell idx = (i, j, k), corrected by the scalar behind `acc` on the interior set (`in`) and handed on off it:
//   g = x[+1]_a - x[-1]_a;  g = g * h_a;  g = scale * g;  v = U_a - g
// the old value is touched once (non-temporal), the scalar's neighbours are plain loads
template <typename T>
__device__ __forceinline__ T proj_corrected(const DevGeom& G, const ProjVec<T>& U, const FieldAcc<T>& acc, T scale, int a,
                                            int64_t idx, int64_t i, int64_t j, int64_t k, bool in) {
  T v = __builtin_nontemporal_load(U.v[a].p + idx);
  if (in) {
    T xp, xm;
    pa_nbrs<T>(G, acc, a, i, j, k, xp, xm);
    T g = xp - xm;
    g = g * U.h[a];
    g = scale * g;
    v = v - g;
  }
  return v;
}

// [p, p + pbytes) against the buffers of a call, each `bbytes` long (null entries: not part of the call)
static inline bool overlaps(const void* p, size_t pbytes, std::initializer_list<const void*> bufs, size_t bbytes) {
  for (const void* b : bufs)
    if (p && b && (const char*)p < (const char*)b + bbytes && (const char*)b < (const char*)p + pbytes) return true;
  return false;
}

// the refusals the entry points share, made before anything is enqueued
static inline int check_projection_call(pa_ctx* c, const char* who, int ncomp) {
  if (!c || !c->grid_set) return PA_E_STATE;
  if (c->slab || (c->G.n0 != c->G.g0 && c->ndim == 3)) { pa_set_err(c, "%s: single GPU only (no slabs)", who); return PA_E_STATE; }
  if (c->solve != PA_SOLVE_NONE) { pa_set_err(c, "%s during a stepwise solve (pa_cg_begin ... pa_cg_end); end or abort it first", who); return PA_E_STATE; }
  if (c->coord != PA_COORD_XYZ) { pa_set_err(c, "%s: for xyz meshes (no axisymmetric rows)", who); return PA_E_ARG; }
  if (c->ndim < 2 || ncomp != c->ndim) {
    pa_set_err(c, "%s: one component per mesh axis on a 2-D or 3-D mesh (%d components, %d axes)", who, ncomp, c->ndim);
    return PA_E_ARG;
  }
  return PA_OK;
}
