// lds_union_find.h -- the lock-free union-find over positions of a unit's member list, its parents in LDS (device code only): what
// set_modules.hip's component search and seed_connect.hip's first components share.  The larger root is hooked under the smaller with a
// compare-and-swap, finds halve their path; a root is therefore the smallest position of its component.  uf_flatten then points every
// position at its root.
#pragma once
#include "common.h"

namespace gss {
namespace {   // as device_scope.h: every file that includes this has its own copy and the library exports nothing from here

__device__ __forceinline__ int32_t uf_find(volatile int32_t *parent, int32_t x) {
  // path halving: a non-root's parent is only ever replaced by one of its ancestors, and ancestors stay ancestors (only roots get
  // hooked), so a racing plain store never detaches anything; parents only decrease, so there are no cycles
  for (;;) {
    const int32_t p = parent[x];
    if (p == x) return x;
    const int32_t g = parent[p];
    if (g == p) return p;
    parent[x] = g;
    x = g;
  }
}

__device__ __forceinline__ void uf_union(int32_t *parent, int32_t a, int32_t b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    const int32_t hi = max(a, b), lo = min(a, b);
    if (atomicCAS(&parent[hi], hi, lo) == hi) return;   // lost: hi was hooked by another lane meanwhile; look again
  }
}

// Pointer jumping over parent[0 .. m) by the nt threads of the workgroup until no parent changes: every parent is then its component's
// root.  A racing read sees an ancestor either way.  Starts after a barrier of the caller's, ends in one
__device__ __forceinline__ void uf_flatten(int32_t *parent, int32_t m, int32_t tid, int32_t nt) {
  for (;;) {
    int moved = 0;
    for (int32_t i = tid; i < m; i += nt) {
      const int32_t p = parent[i], g = ((volatile int32_t *)parent)[p];
      if (g != p) {
        ((volatile int32_t *)parent)[i] = g;
        moved = 1;
      }
    }
    if (!__syncthreads_or(moved)) break;
  }
}

}  // namespace
}  // namespace gss
