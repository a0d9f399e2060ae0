// k_ep_*: what TrackMLDataset.__getitem__ (reference Modules/utils.py:57-108) does to one event, on the device.
//
// node stage (N hits)
//   k_ep_touch     one thread per id of edge_index: touched[id] = 1 (a byte; every writer stores the same value), an id
//                  outside [0, N) sets HGNN_EP_ST_BAD_ID instead.  No sort, no unique.
//   exclusive scan (rocprim, int32) of keep[i] over a transform iterator -- no flag array -- into new_id
//   k_ep_node_fill new_id[i] = keep ? position : -1, pt_out[i] = pid == 0 ? 0 : pt, the last thread writes N'
//   nhits          stable rocprim::radix_sort_pairs of (pid, position) over the 64 key bits, inclusive scan of the run
//                  heads = the run number of every sorted slot, k_ep_run_starts (first slot of every run),
//                  k_ep_run_scatter (nhits[position] = run length; signal_mask from it)
// edge stage (one list of E edges)
//   exclusive scan of "both ends kept, edge_keep set" over a transform iterator into pos (workspace),
//   k_ep_edge_count (count, status), then, once the caller knows the count, k_ep_edge_fill: (new_id[a], new_id[b]), y
//   and y_pid at pos[e].  Output order = input order.
// k_ep_inverse_mask, k_ep_gather: the kept positions and the row compaction of a node field through them.
//
// Every kernel is memory-bound: block 256, at most kEpMaxBlocks workgroups, grid-stride.  An id is compared with
// [0, N) before it forms an address.  The only atomic is an integer OR into the status word.
#include "common.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace hgnn {
namespace {

constexpr int64_t kEpMax = ((int64_t)1 << 31) - 1;          // N, E: positions are int32
constexpr int64_t kEpMaxBlocks = 2048;

unsigned ep_grid(int64_t n) {
    const int64_t b = ceil_div(n > 0 ? n : 1, kBlock);
    return (unsigned)(b < kEpMaxBlocks ? b : kEpMaxBlocks);
}

#define EP_FOR(i, n) \
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < (n); i += (int64_t)gridDim.x * kBlock)

using EpCount = rocprim::counting_iterator<int32_t>;

// keep[i] of the node stage
struct EpKeepNode {
    const int64_t* pid;
    const float* pt;
    const uint8_t* touched;      // NULL: remove_isolated off
    int noise, cut_on;
    float cut;
    __host__ __device__ __forceinline__ int32_t operator()(const int32_t& i) const {
        bool k = noise || pid[i] != 0;
        if (cut_on) k = k && pt[i] > cut;                       // false for NaN
        if (touched != nullptr) k = k && touched[i] != 0;
        return k ? 1 : 0;
    }
};

// 1 where sorted slot j starts a run of equal keys
struct EpRunHead {
    const int64_t* key;
    __host__ __device__ __forceinline__ int32_t operator()(const int32_t& j) const {
        return j == 0 || key[j] != key[j - 1] ? 1 : 0;
    }
};

// edge e survives: both ends in range and kept, the caller's keep byte set
struct EpKeepEdge {
    const int64_t* edges;
    int64_t E, N;
    const int32_t* new_id;
    const uint8_t* edge_keep;    // NULL: all
    __host__ __device__ __forceinline__ int32_t operator()(const int32_t& e) const {
        const int64_t a = edges[e], b = edges[E + e];
        if (a < 0 || a >= N || b < 0 || b >= N) return 0;
        if (edge_keep != nullptr && edge_keep[e] == 0) return 0;
        return new_id[a] >= 0 && new_id[b] >= 0 ? 1 : 0;
    }
};

__device__ __forceinline__ void ep_flag(int64_t* status, int64_t bit) {
    atomicOr((unsigned long long*)status, (unsigned long long)bit);
}

__global__ __launch_bounds__(kBlock) void k_ep_touch(const int64_t* __restrict__ ids, int64_t n_ids, int64_t N,
                                                     uint8_t* __restrict__ touched, int64_t* __restrict__ status) {
    bool bad = false;
    EP_FOR(t, n_ids) {
        const int64_t v = ids[t];
        if (v >= 0 && v < N) touched[v] = 1;
        else bad = true;
    }
    if (bad) ep_flag(status, HGNN_EP_ST_BAD_ID);
}

// new_id holds the exclusive scan of keep on entry
__global__ __launch_bounds__(kBlock) void k_ep_node_fill(EpKeepNode keep, int64_t N, int32_t* __restrict__ new_id,
                                                         float* __restrict__ pt_out, int64_t* __restrict__ n_kept) {
    EP_FOR(i, N) {
        const int32_t k = keep((int32_t)i), p = new_id[i];
        if (i == N - 1) *n_kept = (int64_t)p + k;
        new_id[i] = k ? p : -1;
        pt_out[i] = keep.pid[i] == 0 ? 0.f : keep.pt[i];
    }
}

// run[j]: 1-based run number of sorted slot j; start[r] = first slot of run r (0-based), start[n_runs] = N
__global__ __launch_bounds__(kBlock) void k_ep_run_starts(const int64_t* __restrict__ key,
                                                          const int32_t* __restrict__ run, int64_t N,
                                                          int32_t* __restrict__ start) {
    EP_FOR(j, N) {
        if (j == 0 || key[j] != key[j - 1]) start[run[j] - 1] = (int32_t)j;
        if (j == N - 1) start[run[j]] = (int32_t)N;
    }
}

__global__ __launch_bounds__(kBlock) void k_ep_run_scatter(const int32_t* __restrict__ run,
                                                           const int32_t* __restrict__ start,
                                                           const int32_t* __restrict__ where, int64_t N,
                                                           const int64_t* __restrict__ primary, int64_t n_hits,
                                                           int64_t* __restrict__ nhits,
                                                           uint8_t* __restrict__ signal_mask) {
    EP_FOR(j, N) {
        const int32_t r = run[j], i = where[j];
        const int64_t len = (int64_t)start[r] - (int64_t)start[r - 1];
        nhits[i] = len;
        if (signal_mask != nullptr) signal_mask[i] = len >= n_hits && (primary == nullptr || primary[i] == 1) ? 1 : 0;
    }
}

__global__ __launch_bounds__(kBlock) void k_ep_inverse_mask(const int32_t* __restrict__ new_id, int64_t N,
                                                            int64_t* __restrict__ inverse_mask, int64_t cap) {
    EP_FOR(i, N) {
        const int64_t p = new_id[i];
        if (p >= 0 && p < cap) inverse_mask[p] = i;
    }
}

__global__ __launch_bounds__(kBlock) void k_ep_edge_count(EpKeepEdge keep, const int32_t* __restrict__ pos,
                                                          int64_t* __restrict__ count, int64_t* __restrict__ status) {
    bool bad = false;
    EP_FOR(e, keep.E) {
        const int64_t a = keep.edges[e], b = keep.edges[keep.E + e];
        if (a < 0 || a >= keep.N || b < 0 || b >= keep.N) bad = true;
        if (e == keep.E - 1) *count = (int64_t)pos[e] + keep((int32_t)e);
    }
    if (bad) ep_flag(status, HGNN_EP_ST_BAD_ID);
}

__global__ __launch_bounds__(kBlock) void k_ep_edge_fill(EpKeepEdge keep, const int32_t* __restrict__ pos,
                                                         const uint8_t* __restrict__ y,
                                                         const uint8_t* __restrict__ y_pid, int64_t* __restrict__ out,
                                                         int64_t cap, uint8_t* __restrict__ y_out,
                                                         uint8_t* __restrict__ y_pid_out) {
    EP_FOR(e, keep.E) {
        if (!keep((int32_t)e)) continue;
        const int64_t p = pos[e];
        if (p < 0 || p >= cap) continue;
        out[p] = keep.new_id[keep.edges[e]];
        out[cap + p] = keep.new_id[keep.edges[keep.E + e]];
        if (y_out != nullptr) y_out[p] = y[e];
        if (y_pid_out != nullptr) y_pid_out[p] = y_pid[e];
    }
}

template <class T>
__global__ __launch_bounds__(kBlock) void k_ep_gather(const T* __restrict__ src, int64_t n_rows, int32_t cols,
                                                      const int64_t* __restrict__ index, int64_t n_out,
                                                      T* __restrict__ out) {
    const int64_t total = n_out * cols;
    EP_FOR(t, total) {
        const int64_t r = t / cols, c = t - r * cols, s = index[r];
        out[t] = s >= 0 && s < n_rows ? src[s * cols + c] : (T)0;
    }
}

// ------------------------------------------------------------------ workspaces
struct EpHitWorkspace {
    size_t key, where, run, start, temp, temp_bytes, total;
};

struct EpTake {
    size_t off = 0;
    size_t operator()(size_t bytes) {
        const size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    }
};

// rocprim's scratch sizes are asked for once per size and device (as gc_layout in graphcon.hip does): a dataset
// repeats its shapes, and every entry lays its workspace out again
struct EpSizeCache {
    int64_t n = -1;
    int dev = -1;
    size_t bytes = 0;
    bool hit(int64_t n_, int* dev_) const {
        if (hipGetDevice(dev_) != hipSuccess) *dev_ = -1;     // no device: the size query reports it
        return *dev_ >= 0 && *dev_ == dev && n_ == n;
    }
    void set(int64_t n_, int dev_, size_t b) { n = n_, dev = dev_, bytes = b; }
};

int ep_hit_layout(int64_t N, EpHitWorkspace* w, size_t base, hipStream_t stream) {
    thread_local EpSizeCache cache;
    size_t t1 = 0, t2 = 0;
    int dev = -1;
    if (N > 0 && cache.hit(N, &dev)) {
        t1 = cache.bytes;
    } else if (N > 0) {
        HGNN_CHECK_HIP(rocprim::radix_sort_pairs(nullptr, t1, (const int64_t*)nullptr, (int64_t*)nullptr, EpCount(0),
                                                 (int32_t*)nullptr, (size_t)N, 0u, 64u, stream));
        HGNN_CHECK_HIP(rocprim::inclusive_scan(nullptr, t2,
                                               rocprim::make_transform_iterator(EpCount(0), EpRunHead{nullptr}),
                                               (int32_t*)nullptr, (size_t)N, rocprim::plus<int32_t>(), stream));
        cache.set(N, dev, t1 > t2 ? t1 : t2);
    }
    EpTake take;
    take.off = base;
    const size_t n = (size_t)N;
    w->key = take(n * 8);
    w->where = take(n * 4);
    w->run = take(n * 4);
    w->start = take((n + 1) * 4);
    w->temp_bytes = t1 > t2 ? t1 : t2;
    w->temp = take(w->temp_bytes + 256);
    w->total = take.off;
    return HGNN_OK;
}

// nhits (and signal_mask) out of a workspace laid out by ep_hit_layout; N > 0
int ep_hit_counts(const int64_t* pid, const int64_t* primary, int64_t N, int64_t n_hits, int64_t* nhits,
                  uint8_t* signal_mask, char* ws, const EpHitWorkspace& w, hipStream_t stream) {
    int64_t* key = (int64_t*)(ws + w.key);
    int32_t *where = (int32_t*)(ws + w.where), *run = (int32_t*)(ws + w.run), *start = (int32_t*)(ws + w.start);
    void* temp = ws + w.temp;
    size_t tb = w.temp_bytes;
    HGNN_CHECK_HIP(rocprim::radix_sort_pairs(temp, tb, pid, key, EpCount(0), where, (size_t)N, 0u, 64u, stream));
    tb = w.temp_bytes;
    HGNN_CHECK_HIP(rocprim::inclusive_scan(temp, tb, rocprim::make_transform_iterator(EpCount(0), EpRunHead{key}), run,
                                           (size_t)N, rocprim::plus<int32_t>(), stream));
    k_ep_run_starts<<<ep_grid(N), kBlock, 0, stream>>>(key, run, N, start);
    k_ep_run_scatter<<<ep_grid(N), kBlock, 0, stream>>>(run, start, where, N, primary, n_hits, nhits, signal_mask);
    return HGNN_OK;
}

struct EpNodeWorkspace {
    size_t touched, temp, temp_bytes, total;
    EpHitWorkspace hit;
};

int ep_node_layout(int64_t N, EpNodeWorkspace* w, hipStream_t stream) {
    thread_local EpSizeCache cache;
    size_t t = 0;
    int dev = -1;
    if (N > 0 && cache.hit(N, &dev)) {
        t = cache.bytes;
    } else if (N > 0) {
        HGNN_CHECK_HIP(rocprim::exclusive_scan(
            nullptr, t, rocprim::make_transform_iterator(EpCount(0), EpKeepNode{nullptr, nullptr, nullptr, 0, 0, 0.f}),
            (int32_t*)nullptr, (int32_t)0, (size_t)N, rocprim::plus<int32_t>(), stream));
        cache.set(N, dev, t);
    }
    EpTake take;
    w->touched = take((size_t)N);
    w->temp_bytes = t;
    w->temp = take(t + 256);
    int rc = ep_hit_layout(N, &w->hit, take.off, stream);
    if (rc != HGNN_OK) return rc;
    w->total = w->hit.total;
    return HGNN_OK;
}

struct EpEdgeWorkspace {
    size_t pos, temp, temp_bytes, total;
};

int ep_edge_layout(int64_t E, EpEdgeWorkspace* w, hipStream_t stream) {
    thread_local EpSizeCache cache;
    size_t t = 0;
    int dev = -1;
    if (E > 0 && cache.hit(E, &dev)) {
        t = cache.bytes;
    } else if (E > 0) {
        HGNN_CHECK_HIP(rocprim::exclusive_scan(
            nullptr, t, rocprim::make_transform_iterator(EpCount(0), EpKeepEdge{nullptr, 0, 0, nullptr, nullptr}),
            (int32_t*)nullptr, (int32_t)0, (size_t)E, rocprim::plus<int32_t>(), stream));
        cache.set(E, dev, t);
    }
    EpTake take;
    w->pos = take((size_t)E * 4);
    w->temp_bytes = t;
    w->temp = take(t + 256);
    w->total = take.off;
    return HGNN_OK;
}

int ep_check_sizes(const char* who, int64_t N, int64_t E) {
    HGNN_REQUIRE(N >= 0 && N <= kEpMax, "%s: N = %lld outside [0, 2^31)", who, (long long)N);
    HGNN_REQUIRE(E >= 0 && E <= kEpMax, "%s: E = %lld outside [0, 2^31)", who, (long long)E);
    return HGNN_OK;
}

}  // namespace
}  // namespace hgnn

using namespace hgnn;

extern "C" int hgnn_event_hit_counts_workspace_bytes(int64_t N, size_t* bytes) {
    const char* who = "hgnn_event_hit_counts_workspace_bytes";
    HGNN_REQUIRE(bytes != nullptr, "%s: bytes is NULL", who);
    int rc = ep_check_sizes(who, N, 0);
    if (rc != HGNN_OK) return rc;
    EpHitWorkspace w;
    rc = ep_hit_layout(N, &w, 0, nullptr);
    if (rc != HGNN_OK) return rc;
    *bytes = w.total;
    return HGNN_OK;
}

extern "C" int hgnn_event_hit_counts(const int64_t* pid, const int64_t* primary, int64_t N, int64_t n_hits,
                                     int64_t* nhits, uint8_t* signal_mask, void* workspace, size_t workspace_bytes,
                                     hgnn_stream_t stream_) {
    const char* who = "hgnn_event_hit_counts";
    hipStream_t stream = (hipStream_t)stream_;
    int rc = ep_check_sizes(who, N, 0);
    if (rc != HGNN_OK) return rc;
    if (N == 0) return HGNN_OK;
    HGNN_REQUIRE(pid != nullptr && nhits != nullptr, "%s: NULL pointer", who);
    EpHitWorkspace w;
    rc = ep_hit_layout(N, &w, 0, stream);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE_WORKSPACE(who, workspace, workspace_bytes, w.total);
    rc = ep_hit_counts(pid, primary, N, n_hits, nhits, signal_mask, (char*)workspace, w, stream);
    if (rc != HGNN_OK) return rc;
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}

extern "C" int hgnn_event_nodes_workspace_bytes(int64_t N, int64_t E, size_t* bytes) {
    const char* who = "hgnn_event_nodes_workspace_bytes";
    HGNN_REQUIRE(bytes != nullptr, "%s: bytes is NULL", who);
    int rc = ep_check_sizes(who, N, E);
    if (rc != HGNN_OK) return rc;
    EpNodeWorkspace w;
    rc = ep_node_layout(N, &w, nullptr);
    if (rc != HGNN_OK) return rc;
    *bytes = w.total;
    return HGNN_OK;
}

extern "C" int hgnn_event_nodes(const int64_t* pid, const float* pt, const int64_t* primary,
                                const int64_t* edge_index, int64_t N, int64_t E, double hard_ptcut, int64_t n_hits,
                                int32_t flags, int32_t* new_id, float* pt_out, int64_t* nhits, uint8_t* signal_mask,
                                int64_t* info, void* workspace, size_t workspace_bytes, hgnn_stream_t stream_) {
    const char* who = "hgnn_event_nodes";
    hipStream_t stream = (hipStream_t)stream_;
    int rc = ep_check_sizes(who, N, E);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE((flags & ~(HGNN_EP_NOISE | HGNN_EP_REMOVE_ISOLATED | HGNN_EP_USE_PRIMARY)) == 0,
                 "%s: unknown flag bits", who);
    HGNN_REQUIRE(info != nullptr, "%s: info is NULL", who);
    const bool isolated = (flags & HGNN_EP_REMOVE_ISOLATED) != 0, use_primary = (flags & HGNN_EP_USE_PRIMARY) != 0;
    if (N > 0) {
        HGNN_REQUIRE(pid && pt && new_id && pt_out && nhits && signal_mask, "%s: NULL pointer", who);
        HGNN_REQUIRE(!use_primary || primary != nullptr, "%s: HGNN_EP_USE_PRIMARY needs primary", who);
        HGNN_REQUIRE(!isolated || E == 0 || edge_index != nullptr, "%s: HGNN_EP_REMOVE_ISOLATED needs edge_index",
                     who);
    }
    EpNodeWorkspace w;
    rc = ep_node_layout(N, &w, stream);
    if (rc != HGNN_OK) return rc;
    if (N > 0) HGNN_REQUIRE_WORKSPACE(who, workspace, workspace_bytes, w.total);
    HGNN_CHECK_HIP(hipMemsetAsync(info, 0, HGNN_EP_INFO * sizeof(int64_t), stream));
    if (N == 0) return HGNN_OK;
    char* ws = (char*)workspace;
    uint8_t* touched = nullptr;
    if (isolated) {
        touched = (uint8_t*)(ws + w.touched);
        HGNN_CHECK_HIP(hipMemsetAsync(touched, 0, (size_t)N, stream));
        if (E > 0) k_ep_touch<<<ep_grid(2 * E), kBlock, 0, stream>>>(edge_index, 2 * E, N, touched,
                                                                    info + HGNN_EP_STATUS);
    }
    const EpKeepNode keep{pid, pt, touched, (flags & HGNN_EP_NOISE) != 0, hard_ptcut > 0.0, (float)hard_ptcut};
    size_t tb = w.temp_bytes;
    HGNN_CHECK_HIP(rocprim::exclusive_scan(ws + w.temp, tb, rocprim::make_transform_iterator(EpCount(0), keep), new_id,
                                           (int32_t)0, (size_t)N, rocprim::plus<int32_t>(), stream));
    k_ep_node_fill<<<ep_grid(N), kBlock, 0, stream>>>(keep, N, new_id, pt_out, info + HGNN_EP_N_NODES);
    rc = ep_hit_counts(pid, use_primary ? primary : nullptr, N, n_hits, nhits, signal_mask, ws, w.hit, stream);
    if (rc != HGNN_OK) return rc;
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}

extern "C" int hgnn_event_inverse_mask(const int32_t* new_id, int64_t N, int64_t* inverse_mask, int64_t cap,
                                       hgnn_stream_t stream_) {
    const char* who = "hgnn_event_inverse_mask";
    int rc = ep_check_sizes(who, N, 0);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE(cap >= 0, "%s: need cap >= 0", who);
    if (N == 0 || cap == 0) return HGNN_OK;
    HGNN_REQUIRE(new_id != nullptr && inverse_mask != nullptr, "%s: NULL pointer", who);
    k_ep_inverse_mask<<<ep_grid(N), kBlock, 0, (hipStream_t)stream_>>>(new_id, N, inverse_mask, cap);
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}

extern "C" int hgnn_event_edges_workspace_bytes(int64_t E, size_t* bytes) {
    const char* who = "hgnn_event_edges_workspace_bytes";
    HGNN_REQUIRE(bytes != nullptr, "%s: bytes is NULL", who);
    int rc = ep_check_sizes(who, 0, E);
    if (rc != HGNN_OK) return rc;
    EpEdgeWorkspace w;
    rc = ep_edge_layout(E, &w, nullptr);
    if (rc != HGNN_OK) return rc;
    *bytes = w.total;
    return HGNN_OK;
}

extern "C" int hgnn_event_edges_count(const int64_t* edges, int64_t E, const uint8_t* edge_keep, const int32_t* new_id,
                                      int64_t N, int64_t* count, int64_t* status, void* workspace,
                                      size_t workspace_bytes, hgnn_stream_t stream_) {
    const char* who = "hgnn_event_edges_count";
    hipStream_t stream = (hipStream_t)stream_;
    int rc = ep_check_sizes(who, N, E);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE(count != nullptr && status != nullptr, "%s: count or status is NULL", who);
    HGNN_CHECK_HIP(hipMemsetAsync(count, 0, sizeof(int64_t), stream));
    if (E == 0) return HGNN_OK;
    HGNN_REQUIRE(edges != nullptr && (N == 0 || new_id != nullptr), "%s: NULL pointer", who);
    EpEdgeWorkspace w;
    rc = ep_edge_layout(E, &w, stream);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE_WORKSPACE(who, workspace, workspace_bytes, w.total);
    char* ws = (char*)workspace;
    int32_t* pos = (int32_t*)(ws + w.pos);
    const EpKeepEdge keep{edges, E, N, new_id, edge_keep};
    size_t tb = w.temp_bytes;
    HGNN_CHECK_HIP(rocprim::exclusive_scan(ws + w.temp, tb, rocprim::make_transform_iterator(EpCount(0), keep), pos,
                                           (int32_t)0, (size_t)E, rocprim::plus<int32_t>(), stream));
    k_ep_edge_count<<<ep_grid(E), kBlock, 0, stream>>>(keep, pos, count, status);
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}

extern "C" int hgnn_event_edges_fill(const int64_t* edges, int64_t E, const uint8_t* edge_keep, const int32_t* new_id,
                                     int64_t N, const uint8_t* y, const uint8_t* y_pid, int64_t* out, int64_t cap,
                                     uint8_t* y_out, uint8_t* y_pid_out, const void* workspace, size_t workspace_bytes,
                                     hgnn_stream_t stream_) {
    const char* who = "hgnn_event_edges_fill";
    hipStream_t stream = (hipStream_t)stream_;
    int rc = ep_check_sizes(who, N, E);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE(cap >= 0, "%s: need cap >= 0", who);
    if (E == 0 || cap == 0 || N == 0) return HGNN_OK;
    HGNN_REQUIRE(edges != nullptr && new_id != nullptr && out != nullptr, "%s: NULL pointer", who);
    HGNN_REQUIRE((y_out == nullptr || y != nullptr) && (y_pid_out == nullptr || y_pid != nullptr),
                 "%s: y_out / y_pid_out without y / y_pid", who);
    EpEdgeWorkspace w;
    rc = ep_edge_layout(E, &w, stream);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE_WORKSPACE(who, workspace, workspace_bytes, w.total);
    const int32_t* pos = (const int32_t*)((const char*)workspace + w.pos);
    const EpKeepEdge keep{edges, E, N, new_id, edge_keep};
    k_ep_edge_fill<<<ep_grid(E), kBlock, 0, stream>>>(keep, pos, y, y_pid, out, cap, y_out, y_pid_out);
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}

extern "C" int hgnn_event_gather_rows(const void* src, int64_t n_rows, int32_t cols, int32_t elem_bytes,
                                      const int64_t* index, int64_t n_out, void* out, hgnn_stream_t stream_) {
    const char* who = "hgnn_event_gather_rows";
    hipStream_t stream = (hipStream_t)stream_;
    HGNN_REQUIRE(n_rows >= 0 && n_rows <= kEpMax && n_out >= 0 && n_out <= kEpMax, "%s: n_rows, n_out outside [0, 2^31)",
                 who);
    HGNN_REQUIRE(cols >= 0, "%s: need cols >= 0", who);
    HGNN_REQUIRE(elem_bytes == 1 || elem_bytes == 4 || elem_bytes == 8, "%s: elem_bytes must be 1, 4 or 8", who);
    if (n_out == 0 || cols == 0) return HGNN_OK;
    HGNN_REQUIRE(index != nullptr && out != nullptr && (n_rows == 0 || src != nullptr), "%s: NULL pointer", who);
    const unsigned grid = ep_grid(n_out * cols);
    if (elem_bytes == 1)
        k_ep_gather<uint8_t><<<grid, kBlock, 0, stream>>>((const uint8_t*)src, n_rows, cols, index, n_out,
                                                          (uint8_t*)out);
    else if (elem_bytes == 4)
        k_ep_gather<uint32_t><<<grid, kBlock, 0, stream>>>((const uint32_t*)src, n_rows, cols, index, n_out,
                                                           (uint32_t*)out);
    else
        k_ep_gather<uint64_t><<<grid, kBlock, 0, stream>>>((const uint64_t*)src, n_rows, cols, index, n_out,
                                                           (uint64_t*)out);
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}
