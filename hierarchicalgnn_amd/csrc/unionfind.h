// The lock-free min-root union-find of hgnn_cc_labels (cluster.hip), shared with the score-cut scan (trackscan.hip).
//
// parent[] is read and written by every workgroup while links are made by atomicCAS: relaxed agent-scope atomics keep
// the compiler from caching entries in registers and the loads out of the per-CU vector cache.  A stale value would
// still be harmless (links are never removed and every link is validated by its CAS).  Every loop has a strictly
// decreasing quantity (vertex id while climbing to a root, candidate root id after a failed CAS), so a grid drains.
#pragma once
#include "common.h"

namespace hgnn {

__device__ __forceinline__ int ld_parent(const int* parent, int v) {
    return __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int uf_find(int* parent, int v) {
    // climb to the root; parents always have SMALLER ids, so the walk is finite.  Path halving writes are
    // benign races: they only ever replace the parent of a NON-root by one of its ancestors.
    int p = ld_parent(parent, v);
    while (p != v) {
        const int gp = ld_parent(parent, p);
        if (gp != p) __hip_atomic_store(parent + v, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v = p;
        p = gp;
    }
    return v;
}

// union of the components of u and v: the larger root is hooked under the smaller
__device__ __forceinline__ void uf_union(int* parent, int u, int v) {
    int a = uf_find(parent, u);
    int b = uf_find(parent, v);
    while (a != b) {
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = atomicCAS(&parent[hi], hi, lo);
        if (old == hi) break;  // hi was still a root: now it hangs under lo
        // hi had been linked under `old` (< hi) meanwhile: continue from there; max(a, b) strictly decreases
        a = uf_find(parent, old);
        b = lo;
    }
}

// parent[i] = root of i, once no more links are made: a read-only climb over strictly decreasing ids.  Races with
// other climbers only replace a parent by its root
__device__ __forceinline__ void uf_compress(int* parent, int i) {
    int r = i;
    int p = ld_parent(parent, r);
    while (p != r) {
        r = p;
        p = ld_parent(parent, r);
    }
    __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace hgnn
