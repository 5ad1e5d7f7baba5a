// Lock-free union-find on an int array of parents (instances.hip): an entry is its own index at a root, a smaller index of its
// component elsewhere.  SCOPE: __HIP_MEMORY_SCOPE_WORKGROUP on LDS, __HIP_MEMORY_SCOPE_AGENT on global memory.
#pragma once
#include <hip/hip_runtime.h>

template <int SCOPE>
__device__ __forceinline__ int uf_find(int* L, int x) {
  for (;;) {
    const int p = __hip_atomic_load(L + x, __ATOMIC_RELAXED, SCOPE);
    if (p == x) return x;
    x = p;
  }
}
// joins the components of a and b.  The larger root is pointed at the smaller with atomicMin: parents only ever decrease, so there
// are no cycles and a component's root is its smallest index whatever the order the unions ran in.  When another thread linked that
// root first (the old value is not the root itself) its new parent still has to meet b: once more from there
template <int SCOPE>
__device__ __forceinline__ void uf_union(int* L, int a, int b) {
  for (;;) {
    a = uf_find<SCOPE>(L, a); b = uf_find<SCOPE>(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, SCOPE);
    if (old == a) return;
    a = old;
  }
}
