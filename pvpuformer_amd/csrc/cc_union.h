// Union-find on a pixel grid, shared by the box-prompt labelling (prompt.hip) and the region clean-up (evalbatch.hip, section 9).
// lab[i] is the parent of pixel i; a root points to itself, and parents only ever decrease towards the root, so the root of a
// finished component is its smallest linear index.  The result does not depend on the order in which the unions happen.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ int cc_find(int* __restrict__ lab, int i) {
    // path halving: every visited node is re-pointed to its grandparent (parents only ever decrease towards the root,
    // so a concurrent writer can at worst install another valid ancestor)
    int r = i;
    while (true) {
        const int p = __hip_atomic_load(lab + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == r) return r;
        const int gp = __hip_atomic_load(lab + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (gp != p) __hip_atomic_store(lab + r, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        r = p;
    }
}
__device__ __forceinline__ void cc_union(int* __restrict__ lab, int a, int b) {
    while (true) {
        a = cc_find(lab, a);
        b = cc_find(lab, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }          // a > b: hang the larger root under the smaller
        const int old = atomicMin(lab + a, b);
        if (old == a) return;                                  // a was still a root: linked
        a = old;                                               // somebody re-parented a meanwhile: merge that parent with b
    }
}
