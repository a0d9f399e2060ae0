// Score-cut scan: the tracking metrics of one event at up to 64 score cuts in one call (hgnn_track_scan).
//
// What the reference evaluates one cut at a time (script.py sets "score_cut": 0.7; the candidates are the
// components of the edges with score >= cut, edge_classifier_base.py:157-168, or the pairs with score >= cut,
// bipartite_classification_base.py:262-263) is evaluated here for every cut of a list, with the work that does
// not depend on the cut done once.  Data flow (T = cuts, M or B = items, n = vertices, N = hits):
//
//   cuts        k_ts_sort_cuts: the T cuts in descending order (stable; a NaN cut, which nothing passes, last),
//               with the caller's slot of each.  Everything below works on the sorted cuts; a row is written to
//               its caller's slot
//   items       k_ts_index: idx[i] = the first (highest) sorted cut that item i passes, a binary search in LDS,
//               one byte per item; T = passes none (a NaN score).  The same pass counts, per idx, all items, the
//               kept items and the kept true items in per-block LDS counters flushed with integer atomics;
//               k_ts_prefix turns the counts into "passes cut j" counts
//   particles   te_particle_stage (trackeval_common.h), once
//   per cut j   EDGE: k_ts_hook links only the edges with idx == j into the union-find carried over from the higher
//               cuts (lowering the cut only adds edges; unionfind.h, the lock-free min-root union of
//               hgnn_cc_labels), k_ts_compress, and k_ts_edge_pairs writes (inverse_mask[v], label[v]) for the
//               vertices met so far.  After each step parent[] is what a fresh hgnn_cc_labels at that cut gives:
//               the label of a component is its smallest vertex id whatever the order of the links.
//               PAIR: k_ts_pair_pairs keeps the pairs with idx <= j.
//               Then hgnn_track_eval's pipeline from the candidate runs to the block sums, at CAPACITY (n or B
//               pairs), and k_ts_finalize writes the row
//   none pass   EDGE only: after the last cut the remaining edges with a non-NaN score are linked and evaluated
//               into a scratch row; k_ts_fallback copies it into the row of every cut that no edge passes
//
// Dead pairs.  The host does not know how many pairs a cut has, so every cut is evaluated over all n (or B)
// slots; a slot without a pair is hit 0 with the reserved label INT64_MAX, which sorts last.  k_ts_cand_keep
// never keeps that run, so its pairs end as sentinel contingency keys exactly like the pairs of a candidate
// that fails the size filter, and nothing after the filter sees them.  A cut without any live pair must give
// hgnn_track_eval's n_pairs == 0 row (no reconstructable-particle count): k_ts_finalize reads the smallest
// sorted label, which is the reserved one only when every slot is dead.  A real label equal to the reserved
// one (PAIR mode) sets bit 2 of the status word: HGNN_TE_STATUS = 2.
//
// Numerics: the only floating-point sums are the fixed-order ones of the pipeline; every count is an integer.
#include "trackeval_common.h"
#include "unionfind.h"

#pragma clang fp contract(off)

namespace hgnn {
namespace {

constexpr int kMaxCuts = HGNN_TS_MAX_CUTS;
constexpr int64_t kDead = HGNN_TS_RESERVED_LABEL;
constexpr int kHistRows = 3;             // all items, kept items, kept true items
constexpr int kHistCols = kMaxCuts + 1;  // per first-passed cut; the last column of cnt holds the row total
constexpr int kIndexBlocks = 2048;

struct TsWorkspace {
    TeWorkspace te;
    size_t hit, cand, parent, present, idx, sorted, order, hist, cnt, scratch, total;
};

int ts_layout(int64_t cap, int64_t n_items, int64_t n_vertices, int64_t N, bool edge, TsWorkspace* w,
              hipStream_t stream) {
    int rc = te_layout(cap, N, &w->te, stream);
    if (rc != HGNN_OK) return rc;
    size_t off = w->te.total;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    };
    w->hit = take((size_t)cap * 8);
    w->cand = take((size_t)cap * 8);
    w->parent = take(edge ? (size_t)n_vertices * 4 : 0);
    w->present = take(edge ? (size_t)n_vertices * 4 : 0);
    w->idx = take((size_t)n_items);
    w->sorted = take(kMaxCuts * sizeof(float));
    w->order = take((kMaxCuts + 1) * sizeof(int32_t));  // [kMaxCuts]: the number of non-NaN cuts
    w->hist = take(kHistRows * kHistCols * sizeof(int32_t));
    w->cnt = take(kHistRows * kHistCols * sizeof(int32_t));
    w->scratch = take(HGNN_TS_ROW * sizeof(double));
    w->total = off;
    return HGNN_OK;
}

// descending, stable, NaN last: rank of cut t = the number of cuts that go before it
__global__ __launch_bounds__(64) void k_ts_sort_cuts(const float* __restrict__ cuts, int T, float* __restrict__ sorted,
                                                     int32_t* __restrict__ order) {
    __shared__ float c[kMaxCuts];
    const int t = threadIdx.x;
    if (t < T) c[t] = cuts[t];
    __syncthreads();
    if (t >= T) return;
    const float v = c[t];
    const bool v_nan = v != v;
    int rank = 0, valid = 0;
    for (int u = 0; u < T; ++u) {
        const float w = c[u];
        const bool w_nan = w != w;
        const bool same = w == v || (w_nan && v_nan);
        rank += (w > v || (v_nan && !w_nan) || (same && u < t)) ? 1 : 0;
        valid += w_nan ? 0 : 1;
    }
    sorted[rank] = v;
    order[rank] = t;
    if (t == 0) order[kMaxCuts] = valid;
}

__global__ __launch_bounds__(256) void k_ts_index(const float* __restrict__ score, const uint8_t* __restrict__ truth,
                                                  const uint8_t* __restrict__ keep, int64_t n_items,
                                                  const float* __restrict__ sorted, const int32_t* __restrict__ order,
                                                  int T, uint8_t* __restrict__ idx, int32_t* __restrict__ hist) {
    __shared__ float s_cut[kMaxCuts];
    __shared__ int32_t s_h[kHistRows * kHistCols];
    const int tid = threadIdx.x;
    if (tid < T) s_cut[tid] = sorted[tid];
    for (int i = tid; i < kHistRows * kHistCols; i += 256) s_h[i] = 0;
    __syncthreads();
    const int n_valid = order[kMaxCuts];
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n_items; i += (int64_t)gridDim.x * 256) {
        const float s = score[i];
        int lo = 0, hi = n_valid;  // the first j with s >= s_cut[j]: the predicate is monotone over descending cuts
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s >= s_cut[mid]) hi = mid;
            else lo = mid + 1;
        }
        const int j = lo < n_valid ? lo : T;  // a NaN score passes nothing
        idx[i] = (uint8_t)j;
        atomicAdd(&s_h[j], 1);
        if (truth != nullptr && (keep == nullptr || keep[i] != 0)) {
            atomicAdd(&s_h[kHistCols + j], 1);
            if (truth[i] != 0) atomicAdd(&s_h[2 * kHistCols + j], 1);
        }
    }
    __syncthreads();
    for (int i = tid; i < kHistRows * kHistCols; i += 256)
        if (s_h[i] != 0) atomicAdd(hist + i, s_h[i]);
}

// cnt[k][j] = items of row k that pass sorted cut j; cnt[k][kMaxCuts] = all items of row k
__global__ __launch_bounds__(64) void k_ts_prefix(const int32_t* __restrict__ hist, int T, int32_t* __restrict__ cnt) {
    const int k = threadIdx.x;
    if (k >= kHistRows) return;
    int32_t run = 0;
    for (int j = 0; j < T; ++j) {
        run += hist[k * kHistCols + j];
        cnt[k * kHistCols + j] = run;
    }
    cnt[k * kHistCols + kMaxCuts] = run + hist[k * kHistCols + T];
}

__global__ __launch_bounds__(256) void k_ts_init(int* __restrict__ parent, int* __restrict__ present, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        parent[i] = i;
        present[i] = 0;
    }
}

// links the edges whose first passed cut is j; with rest (after the last cut) the edges that pass none and have a
// non-NaN score.  Vertex ids outside [0, n) are skipped, as in k_cc_hook
__global__ __launch_bounds__(256) void k_ts_hook(const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                 int64_t M, int n, const uint8_t* __restrict__ idx, int j,
                                                 const float* __restrict__ score, bool rest, int* parent,
                                                 int* __restrict__ present) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= M) return;
    if ((int)idx[e] != j) return;
    if (rest) {
        const float s = score[e];
        if (s != s) return;
    }
    const int64_t u64 = src[e], v64 = dst[e];
    if (u64 < 0 || v64 < 0 || u64 >= n || v64 >= n) return;
    present[u64] = 1;
    present[v64] = 1;
    uf_union(parent, (int)u64, (int)v64);
}

__global__ __launch_bounds__(256) void k_ts_compress(int* parent, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) uf_compress(parent, i);
}

__global__ __launch_bounds__(256) void k_ts_edge_pairs(const int64_t* __restrict__ inverse_mask,
                                                       const int* __restrict__ label,
                                                       const int* __restrict__ present, int n,
                                                       int64_t* __restrict__ hit, int64_t* __restrict__ cand) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const bool live = present[v] != 0;
    hit[v] = live ? inverse_mask[v] : 0;
    cand[v] = live ? (int64_t)label[v] : kDead;
}

__global__ __launch_bounds__(256) void k_ts_pair_pairs(const int64_t* __restrict__ hit_in,
                                                       const int64_t* __restrict__ cand_in,
                                                       const uint8_t* __restrict__ idx, int j,
                                                       const int64_t* __restrict__ inverse_mask, int64_t n_vertices,
                                                       int B, int64_t* __restrict__ hit, int64_t* __restrict__ cand,
                                                       int32_t* __restrict__ err) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    int64_t h = 0, c = kDead;
    if ((int)idx[i] <= j) {
        c = cand_in[i];
        if (c == kDead) atomicOr(err, 2);
        h = hit_in[i];
        // an id the mask cannot map becomes a hit id k_te_pair_keys refuses (status bit 1)
        if (inverse_mask != nullptr) h = (h >= 0 && h < n_vertices) ? inverse_mask[h] : -1;
    }
    hit[i] = h;
    cand[i] = c;
}

// k_te_cand_keep, and the run of the reserved label (the dead slots) is never kept
__global__ __launch_bounds__(256) void k_ts_cand_keep(const int64_t* __restrict__ ck,
                                                      const int32_t* __restrict__ cstart,
                                                      const int32_t* __restrict__ crid, int B, float thr,
                                                      int32_t* __restrict__ keep) {
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= B) return;
    const int R = crid[B - 1];
    int k = 0;
    if (r < R) {
        const int b = cstart[r];
        k = (ck[b] != kDead && (float)(cstart[r + 1] - b) >= thr) ? 1 : 0;
    }
    keep[r] = k;
}

// the row of sorted cut j (j == T: the all-edges row, into scratch).  ck[0] is the smallest label of the capacity
// run: the reserved one only when no slot is live, and then the row is hgnn_track_eval's n_pairs == 0 row
__global__ __launch_bounds__(kRedBlocks) void k_ts_finalize(const double* __restrict__ blk_sum,
                                                            const long long* __restrict__ blk_cnt,
                                                            const int32_t* __restrict__ prid,
                                                            const int32_t* __restrict__ kscan,
                                                            const int64_t* __restrict__ ck, int cap, int N,
                                                            const int32_t* __restrict__ err,
                                                            const int32_t* __restrict__ order,
                                                            const int32_t* __restrict__ cnt, int has_truth, int j,
                                                            int T, double* __restrict__ result,
                                                            double* __restrict__ scratch) {
    const bool ran = cap > 0 && N > 0;
    const bool run = ran && ck[0] != kDead;
    const int e = ran ? *err : 0;
    const double status = (e & 2) ? 2.0 : ((e & 1) ? 1.0 : 0.0);
    double* row = scratch;
    if (j < T) {
        const int slot = order[j];
        if (slot < 0 || slot >= T) return;  // never: order is a permutation of 0 .. T - 1
        row = result + (size_t)slot * HGNN_TS_ROW;
    }
    te_finalize_row(blk_sum, blk_cnt, prid, kscan, cap, N, run, status, row);
    if (threadIdx.x != 0) return;
    row[HGNN_TS_N_PASS] = has_truth ? (double)cnt[kHistCols + (j < T ? j : 0)] : 0.0;
    row[HGNN_TS_N_TRUE_PASS] = has_truth ? (double)cnt[2 * kHistCols + (j < T ? j : 0)] : 0.0;
    row[HGNN_TS_N_TRUE] = has_truth ? (double)cnt[2 * kHistCols + kMaxCuts] : 0.0;
}

// the reference's "when no edge passes, use all edges": the metrics of the all-edges row for such cuts
__global__ __launch_bounds__(64) void k_ts_fallback(const int32_t* __restrict__ cnt, const int32_t* __restrict__ order,
                                                    int T, const double* __restrict__ scratch,
                                                    double* __restrict__ result) {
    const int j = threadIdx.x;
    if (j >= T || cnt[j] != 0) return;
    const int slot = order[j];
    if (slot < 0 || slot >= T) return;
    for (int k = 0; k < HGNN_TE_RESULT; ++k) result[(size_t)slot * HGNN_TS_ROW + k] = scratch[k];
}

int ts_check(const char* who, int32_t mode, int64_t n_items, int64_t n_vertices, int64_t n_hits, int32_t n_cuts,
             int64_t* cap) {
    HGNN_REQUIRE(mode == HGNN_TS_EDGE || mode == HGNN_TS_PAIR, "%s: unknown mode %d", who, (int)mode);
    HGNN_REQUIRE(n_cuts >= 1 && n_cuts <= kMaxCuts, "%s: n_cuts %d outside [1, %d]", who, (int)n_cuts, kMaxCuts);
    HGNN_REQUIRE(n_items >= 0 && n_vertices >= 0, "%s: negative size", who);
    HGNN_REQUIRE(n_items < ((int64_t)1 << 31) - 1 && n_vertices < ((int64_t)1 << 31) - 1,
                 "%s: more than 2^31 - 2 items or vertices", who);
    *cap = mode == HGNN_TS_EDGE ? n_vertices : n_items;
    return te_check_sizes(who, *cap, n_hits);
}

}  // namespace
}  // namespace hgnn

using namespace hgnn;

extern "C" int hgnn_track_scan_workspace_bytes(int32_t mode, int64_t n_items, int64_t n_vertices, int64_t n_hits,
                                               int32_t n_cuts, size_t* bytes) {
    int64_t cap = 0;
    int rc = ts_check("hgnn_track_scan_workspace_bytes", mode, n_items, n_vertices, n_hits, n_cuts, &cap);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE(bytes != nullptr, "hgnn_track_scan_workspace_bytes: NULL bytes");
    TsWorkspace w;
    rc = ts_layout(cap, n_items, n_vertices, n_hits, mode == HGNN_TS_EDGE, &w, nullptr);
    if (rc != HGNN_OK) return rc;
    *bytes = w.total;
    return HGNN_OK;
}

extern "C" int hgnn_track_scan(int32_t mode, const int64_t* a, const int64_t* b, int64_t n_items, const float* score,
                               const float* cuts, int32_t n_cuts, const int64_t* inverse_mask, int64_t n_vertices,
                               const uint8_t* truth, const uint8_t* keep, const int64_t* pid, const float* pt,
                               const uint8_t* primary, int64_t n_hits, double pt_cut, double nhits_cut,
                               double majority_cut, double* result, void* workspace, size_t workspace_bytes,
                               hgnn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char* who = "hgnn_track_scan";
    int64_t cap64 = 0;
    int rc = ts_check(who, mode, n_items, n_vertices, n_hits, n_cuts, &cap64);
    if (rc != HGNN_OK) return rc;
    const bool edge = mode == HGNN_TS_EDGE;
    HGNN_REQUIRE(result != nullptr && cuts != nullptr, "%s: NULL result or cuts", who);
    HGNN_REQUIRE(majority_cut > 0.0, "%s: majority_cut must be > 0", who);
    HGNN_REQUIRE(n_items == 0 || (a != nullptr && b != nullptr && score != nullptr), "%s: NULL item arrays", who);
    HGNN_REQUIRE(!edge || n_vertices == 0 || inverse_mask != nullptr, "%s: EDGE mode needs inverse_mask", who);
    HGNN_REQUIRE(n_hits == 0 || (pid != nullptr && pt != nullptr), "%s: NULL event arrays", who);
    HGNN_REQUIRE(cap64 == 0 || n_hits > 0, "%s: %lld vertices or pairs but no hits", who, (long long)cap64);
    HGNN_REQUIRE(keep == nullptr || truth != nullptr, "%s: keep without truth", who);
    TsWorkspace w;
    rc = ts_layout(cap64, n_items, n_vertices, n_hits, edge, &w, stream);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE_WORKSPACE(who, workspace, workspace_bytes, w.total);
    char* ws = (char*)workspace;
    const TePtrs p = te_ptrs(workspace, w.te);
    const int cap = (int)cap64, N = (int)n_hits, T = (int)n_cuts, nv = (int)n_vertices;
    int64_t *hit = (int64_t*)(ws + w.hit), *cand = (int64_t*)(ws + w.cand);
    int *parent = (int*)(ws + w.parent), *present = (int*)(ws + w.present);
    uint8_t* idx = (uint8_t*)(ws + w.idx);
    float* sorted = (float*)(ws + w.sorted);
    int32_t *order = (int32_t*)(ws + w.order), *hist = (int32_t*)(ws + w.hist), *cnt = (int32_t*)(ws + w.cnt);
    double* scratch = (double*)(ws + w.scratch);
    const int has_truth = truth != nullptr ? 1 : 0;

    HGNN_CHECK_HIP(hipMemsetAsync(hist, 0, kHistRows * kHistCols * sizeof(int32_t), stream));
    HGNN_CHECK_HIP(hipMemsetAsync(p.err, 0, sizeof(int32_t), stream));
    k_ts_sort_cuts<<<1, 64, 0, stream>>>(cuts, T, sorted, order);
    if (n_items > 0) {
        const int64_t want = ceil_div(n_items, 256);
        const unsigned grid = (unsigned)(want < kIndexBlocks ? want : kIndexBlocks);
        k_ts_index<<<grid, 256, 0, stream>>>(score, truth, keep, n_items, sorted, order, T, idx, hist);
    }
    k_ts_prefix<<<1, 64, 0, stream>>>(hist, T, cnt);
    if (N > 0) {
        rc = te_particle_stage(p, pid, pt, primary, N, stream);
        if (rc != HGNN_OK) return rc;
    }
    const bool ran = cap > 0 && N > 0;
    if (edge && ran) k_ts_init<<<blocks_for(nv), 256, 0, stream>>>(parent, present, nv);
    const TeParams prm{majority_cut, nhits_cut, majority_cut * nhits_cut, (float)pt_cut, primary != nullptr ? 1 : 0};
    const float thr = (float)(nhits_cut * majority_cut);
    const int steps = edge ? T + 1 : T;  // EDGE: one more for the all-edges row
    for (int j = 0; j < steps; ++j) {
        if (ran) {
            rc = te_clear(p, N, stream);
            if (rc != HGNN_OK) return rc;
            if (edge) {
                if (n_items > 0) {
                    k_ts_hook<<<(unsigned)ceil_div(n_items, 256), 256, 0, stream>>>(a, b, n_items, nv, idx, j, score,
                                                                                   j == T, parent, present);
                    k_ts_compress<<<blocks_for(nv), 256, 0, stream>>>(parent, nv);
                }
                k_ts_edge_pairs<<<blocks_for(nv), 256, 0, stream>>>(inverse_mask, parent, present, nv, hit, cand);
            } else {
                k_ts_pair_pairs<<<blocks_for(cap), 256, 0, stream>>>(a, b, idx, j, inverse_mask, n_vertices, cap, hit,
                                                                     cand, p.err);
            }
            rc = te_candidate_runs(p, cand, cap, stream);
            if (rc != HGNN_OK) return rc;
            k_ts_cand_keep<<<blocks_for(cap), 256, 0, stream>>>(p.ck, p.cstart, p.crid, cap, thr, p.ckeep);
            rc = te_candidate_relabel(p, cap, stream);
            if (rc != HGNN_OK) return rc;
            rc = te_match_stage(p, hit, cap, N, prm, stream);
            if (rc != HGNN_OK) return rc;
        }
        k_ts_finalize<<<1, kRedBlocks, 0, stream>>>(p.blk_sum, p.blk_cnt, p.prid, p.kscan, p.ck, cap, N, p.err, order,
                                                    cnt, has_truth, j, T, result, scratch);
    }
    if (edge) k_ts_fallback<<<1, 64, 0, stream>>>(cnt, order, T, scratch, result);
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}
