// pa_project.h -- what the translation units of the projection layer share (pa_project.hip, pa_stats.hip): the vector operand
// of a one-pass kernel over the components, the launch-log budget, and the refusals made before anything is enqueued.
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
