// Deterministic HDBSCAN* for the embedding stage's validation step (reference GNNEmbedding/embedding_base.py:40-41,
// 267-272: cuml.cluster.HDBSCAN(min_cluster_size, metric='euclidean', cluster_selection_method='eom')).  The
// definition is DESIGN.md section 3 "HDBSCAN" (tests/hdbscan_ref.py restates it in numpy): no tie is broken by
// arrival order, so the labels do not depend on the order of the points.
//
//   k_hdb_core      core2[i] = the min_samples-th smallest d2(i, .), i counted: one query per lane, the points staged
//                   through LDS in tiles, a sorted list of the KP smallest VALUES in registers (no indices needed)
//   k_hdb_nearest   one Boruvka round's all-pairs pass: for every point the smallest (w2, min id, max id) over the
//                   points of OTHER components (tile of points, core2 and component ids in LDS; candidates are
//                   scanned in ascending id, which is ascending (min id, max id) for a fixed point, so a strict
//                   `<` on w2 keeps the smallest key); blockIdx.y slices the candidates.  Epilogue: integer
//                   atomicMin of (w2 bits, min id) on the point's component
//   k_hdb_comp_max  second pass of the component reduce: the smallest max id among the entries that hold the
//                   component's (w2, min id)
//   k_hdb_hook      every component emits its edge (a mutual choice once), and hooks with cluster.hip's lock-free
//                   union-find idiom (larger root under smaller by atomicCAS)
//   k_hdb_compress  component id = smallest vertex id; clears the per-component minima for the next round
//
// The order (w2, min, max) is a strict total order on the edges, so the chosen edges never close a cycle and the
// result is THE minimum spanning tree under it.  One host read per round (the edge count).  d2 is computed with one
// rounded product and one rounded sum per dimension (__fmul_rn / __fadd_rn: no contraction into an fma), so the
// three kernels and the numpy restatement agree to the bit.
//
// The tree stage (N-1 sorted edges -> multi-way dendrogram -> condensed tree -> EOM -> labels) is sequential
// O(N alpha(N)) host C++ in this file (hdb_tree_host): one device-to-host copy of the sorted edges, one
// host-to-device copy of the labels.
#include "common.h"
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>
#include <rocprim/device/device_radix_sort.hpp>

namespace hgnn {
namespace {

constexpr int kHdbTile = 256;
constexpr int kHdbMaxRounds = 22;   // components at least halve every round: N <= 2^21 needs <= 21
constexpr int64_t kHdbMaxN = (int64_t)1 << 21;
constexpr uint64_t kHdbNone = ~(uint64_t)0;

typedef float hdb_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float hdb_d2_term(float d2, float q, float p) {
    const float t = q - p;
    return __fadd_rn(d2, __fmul_rn(t, t));
}

// d2 of the thread's point to the LDS row `p` (DP floats, zero padded: adding +0 leaves d2 unchanged)
template <int DP>
__device__ __forceinline__ float hdb_d2(const float (&qv)[DP], const float* __restrict__ p) {
    float d2 = 0.f;
#pragma unroll
    for (int v = 0; v < DP / 4; ++v) {
        const hdb_f32x4 p4 = *(const hdb_f32x4*)(p + v * 4);
        d2 = hdb_d2_term(d2, qv[v * 4 + 0], p4.x);
        d2 = hdb_d2_term(d2, qv[v * 4 + 1], p4.y);
        d2 = hdb_d2_term(d2, qv[v * 4 + 2], p4.z);
        d2 = hdb_d2_term(d2, qv[v * 4 + 3], p4.w);
    }
    return d2;
}

template <int DP>
__device__ __forceinline__ void hdb_stage(float* tile, const float* __restrict__ x, int64_t base, int n, int D) {
    for (int t = threadIdx.x; t < n * DP; t += kHdbTile) {
        const int pt = t / DP, d = t % DP;
        tile[t] = d < D ? x[(base + pt) * D + d] : 0.f;
    }
}

template <int KP, int DP>
__global__ __launch_bounds__(kHdbTile) void k_hdb_core(const float* __restrict__ x, int64_t N, int D, int k,
                                                       float* __restrict__ core2) {
    __shared__ __attribute__((aligned(16))) float tile[kHdbTile * DP];
    const int64_t q = (int64_t)blockIdx.x * kHdbTile + threadIdx.x;
    const bool active = q < N;
    float qv[DP];
#pragma unroll
    for (int d = 0; d < DP; ++d) qv[d] = (active && d < D) ? x[q * D + d] : 0.f;
    float best[KP];
#pragma unroll
    for (int j = 0; j < KP; ++j) best[j] = INFINITY;
    for (int64_t base = 0; base < N; base += kHdbTile) {
        const int n = (N - base) < kHdbTile ? (int)(N - base) : kHdbTile;
        __syncthreads();
        hdb_stage<DP>(tile, x, base, n, D);
        __syncthreads();
        if (!active) continue;
        for (int j = 0; j < n; ++j) {
            float c = hdb_d2<DP>(qv, tile + j * DP);
            if (c < best[KP - 1]) {
                // sorted insertion with static indexing (the list stays in registers)
#pragma unroll
                for (int s = 0; s < KP; ++s) {
                    const float b = best[s];
                    const bool lt = c < b;
                    best[s] = lt ? c : b;
                    c = lt ? b : c;
                }
            }
        }
    }
    if (active) {
        float r = best[0];
#pragma unroll
        for (int s = 1; s < KP; ++s) r = (s == k - 1) ? best[s] : r;
        core2[q] = r;
    }
}

struct HdbRound {
    const float* x;
    const float* core2;
    const int32_t* comp;
    float* pbw;        // [S][N] per point and slice: the best w2 ...
    int32_t* pbj;      // ... and its other endpoint (-1: none)
    uint64_t* cbest;   // [N] per component (indexed by its smallest vertex): min (w2 bits << 32 | min id)
    int64_t N;
    int64_t slice_len; // multiple of kHdbTile
    int D;
};

template <int DP>
__global__ __launch_bounds__(kHdbTile) void k_hdb_nearest(const HdbRound r) {
    __shared__ __attribute__((aligned(16))) float tile[kHdbTile * DP];
    __shared__ float tcore[kHdbTile];
    __shared__ int32_t tcomp[kHdbTile];
    const int64_t N = r.N;
    const int64_t q = (int64_t)blockIdx.x * kHdbTile + threadIdx.x;
    const bool active = q < N;
    float qv[DP];
#pragma unroll
    for (int d = 0; d < DP; ++d) qv[d] = (active && d < r.D) ? r.x[q * r.D + d] : 0.f;
    const float qcore = active ? r.core2[q] : 0.f;
    const int32_t qcomp = active ? r.comp[q] : -1;
    float bw = INFINITY;
    int32_t bj = -1;
    const int64_t p_begin = (int64_t)blockIdx.y * r.slice_len;
    const int64_t p_end = (p_begin + r.slice_len) < N ? (p_begin + r.slice_len) : N;
    for (int64_t base = p_begin; base < p_end; base += kHdbTile) {
        const int n = (p_end - base) < kHdbTile ? (int)(p_end - base) : kHdbTile;
        __syncthreads();
        hdb_stage<DP>(tile, r.x, base, n, r.D);
        if ((int)threadIdx.x < n) {
            tcore[threadIdx.x] = r.core2[base + threadIdx.x];
            tcomp[threadIdx.x] = r.comp[base + threadIdx.x];
        }
        __syncthreads();
        if (!active) continue;
        for (int j = 0; j < n; ++j) {
            const float d2 = hdb_d2<DP>(qv, tile + j * DP);
            const float w = fmaxf(fmaxf(d2, qcore), tcore[j]);
            // ascending j = ascending (min id, max id) for this point: strict `<` keeps the smallest key
            if (tcomp[j] != qcomp && w < bw) {
                bw = w;
                bj = (int32_t)(base + j);
            }
        }
    }
    if (!active) return;
    const size_t o = (size_t)blockIdx.y * (size_t)N + (size_t)q;
    r.pbw[o] = bw;
    r.pbj[o] = bj;
    if (bj >= 0) {
        const uint32_t mn = (uint32_t)(bj < (int32_t)q ? bj : (int32_t)q);
        const uint64_t key = ((uint64_t)__float_as_uint(bw) << 32) | mn;   // w2 >= 0: the bit pattern is monotone
        unsigned long long* dst = (unsigned long long*)(r.cbest + qcomp);
        // most entries do not improve their component's minimum: look before the atomic
        if (key < __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(dst, (unsigned long long)key);
    }
}

__global__ __launch_bounds__(256) void k_hdb_comp_max(const HdbRound r, int64_t total, uint32_t* __restrict__ cmax) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int32_t j = r.pbj[t];
    if (j < 0) return;
    const int32_t q = (int32_t)(t % r.N);
    const uint32_t mn = (uint32_t)(j < q ? j : q), mx = (uint32_t)(j < q ? q : j);
    const uint64_t key = ((uint64_t)__float_as_uint(r.pbw[t]) << 32) | mn;
    const int32_t c = r.comp[q];
    if (key == r.cbest[c]) atomicMin(cmax + c, mx);
}

__device__ __forceinline__ int hdb_ld(const int* parent, int v) {
    return __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// climb to the root; parents always have smaller ids, so the walk is finite (cluster.hip uf_find)
__device__ __forceinline__ int hdb_find(int* parent, int v) {
    int p = hdb_ld(parent, v);
    while (p != v) {
        const int gp = hdb_ld(parent, p);
        if (gp != p) __hip_atomic_store(parent + v, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v = p;
        p = gp;
    }
    return v;
}

// state[0] = edges emitted so far (unsigned)
__global__ __launch_bounds__(256) void k_hdb_hook(int64_t N, const int32_t* __restrict__ comp,
                                                  const uint64_t* __restrict__ cbest,
                                                  const uint32_t* __restrict__ cmax, int* parent,
                                                  uint64_t* __restrict__ ekey, uint32_t* __restrict__ ew,
                                                  uint32_t* state) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= N || comp[c] != (int32_t)c) return;
    const uint64_t key = cbest[c];
    if (key == kHdbNone) return;   // no other component (the last one), or non-finite input
    const uint32_t mn = (uint32_t)key, mx = cmax[c];
    if ((int64_t)mx >= N) return;   // cannot happen (the entry that set the key also offers its max id); never index with it
    const int32_t cm = comp[mn], cx = comp[mx];
    const int32_t p = cm == (int32_t)c ? cx : cm;
    // a mutual choice (both components picked this edge) is emitted by the smaller component only
    const bool mutual = cbest[p] == key && cmax[p] == mx;
    if (mutual && p < (int32_t)c) return;
    const uint32_t slot = atomicAdd(state, 1u);
    if (slot < (uint32_t)(N - 1)) {   // never out of bounds, whatever the input
        ekey[slot] = ((uint64_t)mn << 32) | mx;
        ew[slot] = (uint32_t)(key >> 32);
    }
    int a = hdb_find(parent, (int)c), b = hdb_find(parent, (int)p);
    while (a != b) {
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = atomicCAS(&parent[hi], hi, lo);
        if (old == hi) break;
        a = hdb_find(parent, old);   // hi was linked under `old` (< hi) meanwhile: max(a, b) strictly decreases
        b = lo;
    }
}

__global__ __launch_bounds__(256) void k_hdb_init(int64_t N, int32_t* __restrict__ comp, int* __restrict__ parent,
                                                  uint64_t* __restrict__ cbest, uint32_t* __restrict__ cmax,
                                                  uint32_t* __restrict__ state) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) state[0] = 0;
    if (i >= N) return;
    comp[i] = (int32_t)i;
    parent[i] = (int)i;
    cbest[i] = kHdbNone;
    cmax[i] = ~0u;
}

__global__ __launch_bounds__(256) void k_hdb_compress(int64_t N, int* parent, int32_t* __restrict__ comp,
                                                      uint64_t* __restrict__ cbest, uint32_t* __restrict__ cmax) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    int r = (int)i;
    int p = hdb_ld(parent, r);
    while (p != r) {   // no more links are made: a read-only climb over strictly decreasing ids
        r = p;
        p = hdb_ld(parent, r);
    }
    comp[i] = r;
    // races with other climbers only replace a parent by its root
    __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    cbest[i] = kHdbNone;
    cmax[i] = ~0u;
}

__global__ __launch_bounds__(256) void k_hdb_emit(int64_t M, const uint64_t* __restrict__ ekey,
                                                  const uint32_t* __restrict__ ew, int64_t* __restrict__ edges,
                                                  float* __restrict__ w2) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= M) return;
    const uint64_t k = ekey[e];
    edges[2 * e] = (int64_t)(k >> 32);
    edges[2 * e + 1] = (int64_t)(uint32_t)k;
    w2[e] = __uint_as_float(ew[e]);
}

// ------------------------------------------------------------------------------------------- tree stage (host)
struct HdbUf {
    std::vector<int32_t> p;
    explicit HdbUf(int64_t n) : p((size_t)n) {
        for (int64_t i = 0; i < n; ++i) p[(size_t)i] = (int32_t)i;
    }
    int32_t find(int32_t a) {
        while (p[a] != a) {
            p[a] = p[p[a]];
            a = p[a];
        }
        return a;
    }
};

inline double hdb_lambda(float w2) { return w2 > 0.f ? 1.0 / std::sqrt((double)w2) : HGNN_HDBSCAN_LAMBDA_DUP; }

// edges (min << 32 | max) sorted by w2 (bit patterns of non-negative floats); labels[n]: -1 noise, clusters
// 0..C-1 by smallest member.  Returns the number of clusters, or -1 when the edges are not a spanning tree.
int64_t hdb_tree_host(const uint64_t* ekey, const uint32_t* ew, int64_t n, int64_t mcs, int64_t* labels) {
    const int64_t m = n - 1;
    HdbUf uf(n);
    // dendrogram: nodes 0..n-1 are the points; internal node v >= n has children kid[kid_begin[v-n] .. kid_begin[v-n+1])
    std::vector<int32_t> node_of((size_t)n), size((size_t)n, 1), kid, kid_begin(1, 0), roots, fill;
    std::vector<int32_t> stamp((size_t)n, -1);   // the level (its first edge) that last touched a union-find root
    std::vector<int32_t> slot((size_t)n, -1);    // new root -> index into `roots` while a level is built
    std::vector<float> level;
    for (int64_t i = 0; i < n; ++i) node_of[(size_t)i] = (int32_t)i;
    std::vector<std::pair<int32_t, int32_t>> old;   // (root, its node) of the sets a level merges
    kid.reserve((size_t)(2 * n));
    for (int64_t e = 0; e < m;) {
        int64_t f = e;
        while (f < m && ew[f] == ew[e]) ++f;
        old.clear();
        for (int64_t t = e; t < f; ++t) {
            const int32_t a = uf.find((int32_t)(ekey[t] >> 32)), b = uf.find((int32_t)(uint32_t)ekey[t]);
            if (a == b) return -1;
            // the root of a merged pair is one of the two, so every root met here was a root when the level began
            if (stamp[a] != (int32_t)e) {
                stamp[a] = (int32_t)e;
                old.emplace_back(a, node_of[a]);
            }
            if (stamp[b] != (int32_t)e) {
                stamp[b] = (int32_t)e;
                old.emplace_back(b, node_of[b]);
            }
            uf.p[a > b ? a : b] = a > b ? b : a;
        }
        // one new node per merged set; its children are the nodes of the sets it swallowed
        roots.clear();
        for (auto& o : old) {
            o.first = uf.find(o.first);
            if (slot[o.first] < 0) {
                slot[o.first] = (int32_t)roots.size();
                roots.push_back(o.first);
            }
        }
        const size_t first_node = level.size();
        fill.assign(roots.size(), 0);
        for (auto& o : old) ++fill[(size_t)slot[o.first]];
        uint32_t bits = ew[e];
        float wl;
        memcpy(&wl, &bits, 4);
        for (size_t g = 0; g < roots.size(); ++g) {
            kid_begin.push_back(kid_begin.back() + fill[g]);
            fill[g] = kid_begin[first_node + g];
            level.push_back(wl);
            size.push_back(0);
        }
        kid.resize((size_t)kid_begin.back());
        for (auto& o : old) {
            const size_t g = (size_t)slot[o.first];
            kid[(size_t)fill[g]++] = o.second;
            size[(size_t)n + first_node + g] += size[(size_t)o.second];
        }
        for (size_t g = 0; g < roots.size(); ++g) {
            node_of[roots[g]] = (int32_t)(n + first_node + g);
            slot[roots[g]] = -1;
        }
        e = f;
    }
    const int64_t n_nodes = n + (int64_t)level.size();
    if (level.empty() || size[(size_t)n_nodes - 1] != n) return -1;
    const int32_t root = (int32_t)(n_nodes - 1);

    // condensed tree, cluster 0 = the root
    std::vector<int32_t> c_parent(1, -1), fell((size_t)n, 0);
    std::vector<double> c_birth(1, 0.0), c_stab(1, 0.0);
    std::vector<std::pair<int32_t, int32_t>> stack(1, {root, 0});
    std::vector<int32_t> lstack;
    while (!stack.empty()) {
        const int32_t node = stack.back().first, c = stack.back().second;
        stack.pop_back();
        const double lam = hdb_lambda(level[(size_t)(node - n)]);
        const int32_t kb = kid_begin[(size_t)(node - n)], ke = kid_begin[(size_t)(node - n) + 1];
        int n_big = 0;
        for (int32_t t = kb; t < ke; ++t) n_big += size[(size_t)kid[t]] >= mcs;
        for (int32_t t = kb; t < ke; ++t) {
            const int32_t k = kid[t];
            if (size[(size_t)k] >= mcs) continue;
            c_stab[c] += (double)size[(size_t)k] * (lam - c_birth[c]);
            lstack.assign(1, k);
            while (!lstack.empty()) {
                const int32_t v = lstack.back();
                lstack.pop_back();
                if (v < n) fell[(size_t)v] = c;
                else
                    for (int32_t u = kid_begin[(size_t)(v - n)]; u < kid_begin[(size_t)(v - n) + 1]; ++u)
                        lstack.push_back(kid[u]);
            }
        }
        for (int32_t t = kb; t < ke; ++t) {
            const int32_t k = kid[t];
            if (size[(size_t)k] < mcs) continue;
            if (n_big >= 2) {
                c_stab[c] += (double)size[(size_t)k] * (lam - c_birth[c]);
                stack.emplace_back(k, (int32_t)c_parent.size());
                c_parent.push_back(c);
                c_birth.push_back(lam);
                c_stab.push_back(0.0);
            } else {
                stack.emplace_back(k, c);
            }
        }
    }
    // EOM: children have larger ids than their parents; sub[c] = selected stability in c's subtree
    const size_t nc = c_parent.size();
    std::vector<double> below(nc, 0.0);
    std::vector<char> has_kids(nc, 0), selected(nc, 0);
    for (size_t c = nc - 1; c >= 1; --c) {
        const bool sel = !has_kids[c] || c_stab[c] >= below[c];
        selected[c] = sel;
        const double sub = sel ? c_stab[c] : below[c];
        below[(size_t)c_parent[c]] += sub;
        has_kids[(size_t)c_parent[c]] = 1;
    }
    // a cluster is labelled by its highest selected ancestor
    std::vector<int32_t> lab_of(nc, -1);
    for (size_t c = 1; c < nc; ++c) {
        const int32_t p = c_parent[c];
        lab_of[c] = lab_of[(size_t)p] >= 0 ? lab_of[(size_t)p] : (selected[c] ? (int32_t)c : -1);
    }
    std::vector<int64_t> number(nc, -1);
    int64_t n_clusters = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int32_t l = lab_of[(size_t)fell[(size_t)i]];
        if (l < 0) {
            labels[i] = -1;
            continue;
        }
        if (number[(size_t)l] < 0) number[(size_t)l] = n_clusters++;
        labels[i] = number[(size_t)l];
    }
    return n_clusters;
}

struct HdbWorkspace {
    size_t comp, parent, pbw, pbj, cbest, cmax, sorted, ekey_t, ew_t, state, temp, temp_bytes, total;
    int slices;
    int64_t slice_len;
};

int hdb_check(const char* who, int64_t N, int32_t D, int32_t mcs, int32_t ms) {
    HGNN_REQUIRE(D >= 1 && D <= 16, "%s: D must be in [1, 16], got %d", who, (int)D);
    HGNN_REQUIRE(mcs >= 2, "%s: min_cluster_size must be >= 2", who);
    HGNN_REQUIRE(ms >= 1 && ms <= 128, "%s: min_samples must be in [1, 128], got %d", who, (int)ms);
    HGNN_REQUIRE(N >= mcs && N >= ms && N >= 2, "%s: N = %lld is below min_cluster_size or min_samples", who, (long long)N);
    HGNN_REQUIRE(N <= kHdbMaxN, "%s: N must not exceed 2^21", who);
    return HGNN_OK;
}

int hdb_layout(int64_t N, HdbWorkspace* w) {
    const int64_t blocks = ceil_div(N, kHdbTile);
    // enough workgroups for the 256 CUs when there are few points: slice every point's candidates
    int64_t s = ceil_div(1024, blocks);
    s = s < 1 ? 1 : (s > 16 ? 16 : s);
    w->slice_len = ceil_div(ceil_div(N, s), kHdbTile) * kHdbTile;
    w->slices = (int)ceil_div(N, w->slice_len);
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += align_up(bytes, 256);
        return at;
    };
    const size_t n = (size_t)N;
    w->comp = take(n * 4);
    w->parent = take(n * 4);
    w->pbw = take(n * 4 * (size_t)w->slices);
    w->pbj = take(n * 4 * (size_t)w->slices);
    w->cbest = take(n * 8);
    w->cmax = take(n * 4);
    w->sorted = take(n * 12);   // uint64 keys [N] directly followed by uint32 w2 bits [N]: one copy to the host
    w->ekey_t = take(n * 8);
    w->ew_t = take(n * 4);
    w->state = take(256);
    size_t t1 = 0, t2 = 0;
    HGNN_CHECK_HIP(rocprim::radix_sort_pairs(nullptr, t1, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr,
                                             (uint32_t*)nullptr, n, 0u, 64u, (hipStream_t)0));
    HGNN_CHECK_HIP(rocprim::radix_sort_pairs(nullptr, t2, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint64_t*)nullptr,
                                             (uint64_t*)nullptr, n, 0u, 32u, (hipStream_t)0));
    w->temp_bytes = t1 > t2 ? t1 : t2;
    w->temp = take(w->temp_bytes);
    w->total = o;
    return HGNN_OK;
}

template <int DP>
void hdb_launch_core(int kp, unsigned blocks, hipStream_t st, const float* x, int64_t N, int D, int k, float* core2) {
    switch (kp) {
        case 8: k_hdb_core<8, DP><<<blocks, kHdbTile, 0, st>>>(x, N, D, k, core2); break;
        case 16: k_hdb_core<16, DP><<<blocks, kHdbTile, 0, st>>>(x, N, D, k, core2); break;
        case 32: k_hdb_core<32, DP><<<blocks, kHdbTile, 0, st>>>(x, N, D, k, core2); break;
        case 64: k_hdb_core<64, DP><<<blocks, kHdbTile, 0, st>>>(x, N, D, k, core2); break;
        default: k_hdb_core<128, DP><<<blocks, kHdbTile, 0, st>>>(x, N, D, k, core2); break;
    }
}

inline int64_t hdb_now_ns() {
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

}  // namespace
}  // namespace hgnn

using namespace hgnn;

extern "C" int hgnn_hdbscan_workspace_bytes(int64_t N, int32_t D, int32_t min_cluster_size, int32_t min_samples,
                                            size_t* bytes) {
    const char* who = "hgnn_hdbscan_workspace_bytes";
    int rc = hdb_check(who, N, D, min_cluster_size, min_samples);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE(bytes != nullptr, "%s: NULL bytes", who);
    HdbWorkspace w;
    rc = hdb_layout(N, &w);
    if (rc != HGNN_OK) return rc;
    *bytes = w.total;
    return HGNN_OK;
}

extern "C" int hgnn_hdbscan_tree_host(const int64_t* edges, const float* w2, int64_t N, int32_t min_cluster_size,
                                      int64_t* labels, int64_t* n_clusters) {
    const char* who = "hgnn_hdbscan_tree_host";
    HGNN_REQUIRE(edges != nullptr && w2 != nullptr && labels != nullptr, "%s: NULL argument", who);
    HGNN_REQUIRE(N >= 2 && N <= kHdbMaxN && min_cluster_size >= 2, "%s: bad sizes", who);
    std::vector<uint64_t> ekey((size_t)N - 1);
    std::vector<uint32_t> ew((size_t)N - 1);
    for (int64_t e = 0; e < N - 1; ++e) {
        const int64_t a = edges[2 * e], b = edges[2 * e + 1];
        HGNN_REQUIRE(a >= 0 && b >= 0 && a < N && b < N && a != b, "%s: edge %lld has a bad endpoint", who, (long long)e);
        HGNN_REQUIRE(w2[e] >= 0.f && (e == 0 || w2[e] >= w2[e - 1]), "%s: w2 must be non-negative and ascending", who);
        ekey[(size_t)e] = ((uint64_t)(a < b ? a : b) << 32) | (uint64_t)(a < b ? b : a);
        memcpy(&ew[(size_t)e], &w2[e], 4);
    }
    const int64_t c = hdb_tree_host(ekey.data(), ew.data(), N, min_cluster_size, labels);
    HGNN_REQUIRE(c >= 0, "%s: the edges are not a spanning tree", who);
    if (n_clusters != nullptr) *n_clusters = c;
    return HGNN_OK;
}

extern "C" int hgnn_hdbscan_f32(const float* points, int64_t N, int32_t D, int32_t min_cluster_size,
                                int32_t min_samples, int64_t* labels, int64_t* mst_edges, float* mst_w2, float* core2,
                                int64_t* info, void* workspace, size_t workspace_bytes, hgnn_stream_t stream_) {
    const char* who = "hgnn_hdbscan_f32";
    hipStream_t stream = (hipStream_t)stream_;
    int rc = hdb_check(who, N, D, min_cluster_size, min_samples);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE(points != nullptr, "%s: NULL points", who);
    HGNN_REQUIRE(labels != nullptr && mst_edges != nullptr && mst_w2 != nullptr && core2 != nullptr,
                 "%s: NULL output", who);
    HdbWorkspace w;
    rc = hdb_layout(N, &w);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE_WORKSPACE(who, workspace, workspace_bytes, w.total);
    const bool stage_sync = info != nullptr && info[HGNN_HDB_STAGE_SYNC] != 0;
    int64_t inf[HGNN_HDB_INFO] = {0};
    char* ws = (char*)workspace;
    int32_t* comp = (int32_t*)(ws + w.comp);
    int* parent = (int*)(ws + w.parent);
    uint64_t* cbest = (uint64_t*)(ws + w.cbest);
    uint32_t* cmax = (uint32_t*)(ws + w.cmax);
    uint64_t* ekey_s = (uint64_t*)(ws + w.sorted);
    uint32_t* ew_s = (uint32_t*)(ws + w.sorted + (size_t)N * 8);
    uint64_t* ekey_t = (uint64_t*)(ws + w.ekey_t);
    uint32_t* ew_t = (uint32_t*)(ws + w.ew_t);
    uint32_t* state = (uint32_t*)(ws + w.state);
    const unsigned nb = (unsigned)ceil_div(N, 256);
    const int DP = D <= 4 ? 4 : (D <= 8 ? 8 : 16);
    const int kp = min_samples <= 8 ? 8 : (min_samples <= 16 ? 16 : (min_samples <= 32 ? 32 : (min_samples <= 64 ? 64 : 128)));

    int64_t t0 = hdb_now_ns();
    k_hdb_init<<<nb, 256, 0, stream>>>(N, comp, parent, cbest, cmax, state);
    if (DP == 4) hdb_launch_core<4>(kp, nb, stream, points, N, D, min_samples, core2);
    else if (DP == 8) hdb_launch_core<8>(kp, nb, stream, points, N, D, min_samples, core2);
    else hdb_launch_core<16>(kp, nb, stream, points, N, D, min_samples, core2);
    HGNN_CHECK_HIP(hipGetLastError());
    if (stage_sync) {
        HGNN_CHECK_HIP(hipStreamSynchronize(stream));
        inf[HGNN_HDB_T_CORE_NS] = hdb_now_ns() - t0;
        t0 = hdb_now_ns();
    }

    HdbRound r;
    r.x = points;
    r.core2 = core2;
    r.comp = comp;
    r.pbw = (float*)(ws + w.pbw);
    r.pbj = (int32_t*)(ws + w.pbj);
    r.cbest = cbest;
    r.N = N;
    r.slice_len = w.slice_len;
    r.D = D;
    const dim3 grid(nb, (unsigned)w.slices);
    const int64_t total = N * w.slices;
    int64_t reads = 0, rounds = 0;
    uint32_t n_edges = 0;
    while ((int64_t)n_edges < N - 1) {
        if (rounds >= kHdbMaxRounds) {
            set_error("%s: the round budget ran out", who);
            return HGNN_ERR_INVALID_ARG;
        }
        if (DP == 4) k_hdb_nearest<4><<<grid, kHdbTile, 0, stream>>>(r);
        else if (DP == 8) k_hdb_nearest<8><<<grid, kHdbTile, 0, stream>>>(r);
        else k_hdb_nearest<16><<<grid, kHdbTile, 0, stream>>>(r);
        k_hdb_comp_max<<<(unsigned)ceil_div(total, 256), 256, 0, stream>>>(r, total, cmax);
        k_hdb_hook<<<nb, 256, 0, stream>>>(N, comp, cbest, cmax, parent, ekey_s, ew_s, state);
        k_hdb_compress<<<nb, 256, 0, stream>>>(N, parent, comp, cbest, cmax);
        HGNN_CHECK_HIP(hipGetLastError());
        const uint32_t before = n_edges;
        HGNN_CHECK_HIP(hipMemcpyAsync(&n_edges, state, 4, hipMemcpyDeviceToHost, stream));
        HGNN_CHECK_HIP(hipStreamSynchronize(stream));
        ++reads;
        inf[HGNN_HDB_T_ROUND0_NS + rounds] = hdb_now_ns() - t0;
        t0 = hdb_now_ns();
        ++rounds;
        if (n_edges == before || (int64_t)n_edges > N - 1) {
            set_error("%s: a round joined nothing (%u of %lld edges): non-finite coordinates?", who, n_edges,
                      (long long)(N - 1));
            return HGNN_ERR_INVALID_ARG;
        }
    }

    // sort by (w2, min, max): two stable passes, least significant key first
    const size_t M = (size_t)(N - 1);
    void* temp = ws + w.temp;
    size_t tb = w.temp_bytes;
    HGNN_CHECK_HIP(rocprim::radix_sort_pairs(temp, tb, ekey_s, ekey_t, ew_s, ew_t, M, 0u, 64u, stream));
    HGNN_CHECK_HIP(rocprim::radix_sort_pairs(temp, tb, ew_t, ew_s, ekey_t, ekey_s, M, 0u, 32u, stream));
    k_hdb_emit<<<(unsigned)ceil_div((int64_t)M, 256), 256, 0, stream>>>((int64_t)M, ekey_s, ew_s, mst_edges, mst_w2);
    HGNN_CHECK_HIP(hipGetLastError());
    if (stage_sync) HGNN_CHECK_HIP(hipStreamSynchronize(stream));

    std::vector<char> host((size_t)N * 12);
    HGNN_CHECK_HIP(hipMemcpyAsync(host.data(), ekey_s, (size_t)N * 12, hipMemcpyDeviceToHost, stream));
    HGNN_CHECK_HIP(hipStreamSynchronize(stream));
    ++reads;
    inf[HGNN_HDB_T_SORT_NS] = hdb_now_ns() - t0;
    t0 = hdb_now_ns();
    std::vector<int64_t> lab((size_t)N);
    const int64_t n_clusters = hdb_tree_host((const uint64_t*)host.data(), (const uint32_t*)(host.data() + (size_t)N * 8),
                                             N, min_cluster_size, lab.data());
    inf[HGNN_HDB_T_TREE_NS] = hdb_now_ns() - t0;
    if (n_clusters < 0) {
        set_error("%s: the device edges are not a spanning tree", who);
        return HGNN_ERR_INVALID_ARG;
    }
    HGNN_CHECK_HIP(hipMemcpyAsync(labels, lab.data(), (size_t)N * 8, hipMemcpyHostToDevice, stream));
    HGNN_CHECK_HIP(hipStreamSynchronize(stream));   // `lab` leaves scope
    ++reads;
    inf[HGNN_HDB_ROUNDS] = rounds;
    inf[HGNN_HDB_HOST_READS] = reads;
    inf[HGNN_HDB_N_CLUSTERS] = n_clusters;
    inf[HGNN_HDB_STAGE_SYNC] = stage_sync;
    if (info != nullptr) memcpy(info, inf, sizeof(inf));
    return HGNN_OK;
}
