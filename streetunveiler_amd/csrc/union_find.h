// union_find.h -- the lock-free union-find cluster.hip (points within a radius) and mesh_post.hip (faces on a common edge) share (device
// code).  The ECL-CC scheme (Jaiganesh & Burtscher, HPDC 2018): parent[i] <= i always, and a root is only ever hooked under a SMALLER
// root, by compare-and-swap, so the root of a finished tree is the smallest index of its component and the labels do not depend on the
// order in which the unions raced.  The only loops on shared state are the walk to a root, which every step shortens, and the retry of
// a hook whose root another lane hooked first; no lane waits for another.
#pragma once
#include "common.h"

namespace sr {

// parent[] is shared by every wave of the kernel that unites: relaxed agent-scope accesses, so that a retry reads memory again and not a register
__device__ __forceinline__ int load_parent(const int* parent, int i) { return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void store_parent(int* parent, int i, int v) { __hip_atomic_store(parent + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of x's tree, with path halving.  parent[i] <= i always, so the walk descends and ends.  The halving store goes to a node that
// has been seen with a parent other than itself: it is no root and never becomes one again, so the store cannot undo a hook (hooks
// write roots only), and what it writes is an ancestor of that node.
__device__ __forceinline__ int find_root(int* parent, int x) {
    int curr = load_parent(parent, x);
    if (curr == x) return x;
    int prev = x;
    for (;;) {
        const int next = load_parent(parent, curr);
        if (next == curr) return curr;
        store_parent(parent, prev, next);
        prev = curr;
        curr = next;
    }
}

// Joins the trees of a and b: the larger root goes under the smaller.  A failed compare-and-swap means the larger one has been hooked
// meanwhile, to something smaller still, which is where the next attempt starts: max(ra, rb) falls with every retry.
__device__ __forceinline__ void unite(int* parent, int a, int b) {
    int ra = find_root(parent, a), rb = find_root(parent, b);
    while (ra != rb) {
        const int hi = max(ra, rb), lo = min(ra, rb);
        const int seen = atomicCAS(parent + hi, hi, lo);
        if (seen == hi) return;
        ra = seen;
        rb = lo;
    }
}

}  // namespace sr
