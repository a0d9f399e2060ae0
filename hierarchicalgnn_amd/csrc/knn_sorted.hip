// Exact fixed-radius kNN, 1 <= K <= 128, over spatially sorted points with tile pruning: the result of
// k_knn_large / k_knn_radius (the K smallest keys (d2, idx) with d2 < r^2) bit for bit, without comparing every
// query with every point.
//
// k_knn_large selects by the 64-bit key (float bits of d2) << 32 | idx, so its result does not depend on the order
// in which candidates are visited.  Here the points are sorted along a Morton curve, cut into tiles of 256 with an
// axis-aligned box each, and a workgroup of 16 curve-consecutive queries visits the tiles from its home tile
// outwards and skips a tile whose box is provably too far to hold a candidate the brute-force kernel would keep.
// Stages, all on the caller's stream, every array in the caller's workspace, no host read:
//
//   bbox     per-dimension min / max of the finite coordinates of points (and of query when it is another array):
//            integer atomicMin / atomicMax on order-preserving float bits (commutative: deterministic)
//   keys     64-bit Morton key of every row over its D real dimensions, min(21, 63 / D) bits per dimension,
//            quantised inside the union of the two boxes; a row with a non-finite coordinate gets the all-ones key
//   sort     stable rocprim::radix_sort_pairs (key, original row); one sort when query IS points
//   gather   sorted zero-padded points [np, DP], perm (original row of each sorted row), per tile lo[DP], hi[DP] over
//            the finite coordinates and the flag "holds a non-finite coordinate: never skip"
//   search   k_knn_sorted<DP>: k_knn_large's wave (4 queries, lanes over the candidates of an LDS tile, ballot-prefix
//            append, lk_flush); the idx inside the key is the ORIGINAL point index (perm is staged with the tile) and
//            row qperm[q] of the outputs is written
//   stats    per workgroup {tiles visited, tiles skipped} -> int64[2] at workspace offset 0 (and stats_out)
//
// THE SKIP RULE.  Each wave decides for its own 4 queries from its own registers (their box wlo / whi, their
// thresholds), then the workgroup skips staging when all four waves skip.  With the tile box tlo / thi,
//     lb = sum_d max(0, tlo_d - whi_d, wlo_d - thi_d)^2        (fp32, fmaf chain in dimension order)
//     bound = max_q min(r2, thr_q)                             (thr_q = 3e38 until query q holds K entries)
//     skip  <=>  tile not flagged  &&  r2 == r2  &&  1e-30 <= lb < inf  &&  lb * 0.9999f > bound
// Every comparison is false on a NaN, so a NaN never skips.  DESIGN.md ("k_knn_sorted") proves that a skipped tile
// holds no candidate whose computed d2 passes `d2 < r2 && d2 <= thr_q` for any of the wave's queries.
//
// d2 is k_knn_large's arithmetic on the same values (zero-padded DP, t = q - p, d2 = fmaf(t, t, d2) in dimension
// order; r2 = r * r in float32; strict d2 < r2; d2 <= thr_q).  No floating-point atomics, no inline assembly.
#include "common.h"
#include "knn_select.h"
#include <rocprim/device/device_radix_sort.hpp>

namespace hgnn {
namespace {

constexpr int kKsGroup = kLkWaves * kLkQ;   // queries per workgroup
constexpr int kKsDMax = 16;
constexpr float kKsSlack = 0.9999f;
constexpr float kKsLbMin = 1e-30f;          // below: squares may be subnormal, relative error bounds do not hold
constexpr uint64_t kKsKeyNonFinite = ~(uint64_t)0;

struct KsWorkspace {
    size_t stats, box, wg, pkey, pkey_s, pval, pperm, qkey, qkey_s, qval, qperm, spts, tlo, thi, tflag, temp,
        temp_bytes, total;
};

int ks_layout(int64_t nq, int64_t np, int DP, KsWorkspace* w, hipStream_t stream) {
    size_t tb = 0;
    for (int64_t n : {nq, np}) {
        size_t t = 0;
        if (n > 0)
            HGNN_CHECK_HIP(rocprim::radix_sort_pairs(nullptr, t, (uint64_t*)nullptr, (uint64_t*)nullptr,
                                                     (int32_t*)nullptr, (int32_t*)nullptr, (size_t)n, 0u, 64u,
                                                     stream));
        tb = t > tb ? t : tb;
    }
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    };
    const size_t q = (size_t)nq, p = (size_t)np, tiles = (size_t)ceil_div(np, kLkTile);
    w->stats = take(2 * sizeof(int64_t));                 // offset 0: {tiles visited, tiles skipped} of the call
    w->box = take(4 * kKsDMax * sizeof(uint32_t));        // min of points, of queries; max of points, of queries
    w->wg = take((size_t)ceil_div(nq, kKsGroup) * 2 * sizeof(int32_t));
    w->pkey = take(p * 8);
    w->pkey_s = take(p * 8);
    w->pval = take(p * 4);
    w->pperm = take(p * 4);
    w->qkey = take(q * 8);
    w->qkey_s = take(q * 8);
    w->qval = take(q * 4);
    w->qperm = take(q * 4);
    w->spts = take(p * DP * 4);
    w->tlo = take(tiles * DP * 4);
    w->thi = take(tiles * DP * 4);
    w->tflag = take(tiles * 4);
    w->temp_bytes = tb;
    w->temp = take(tb + 256);
    w->total = off;
    return HGNN_OK;
}

inline int ks_dp(int D) { return D <= 4 ? 4 : D <= 8 ? 8 : 16; }

__device__ inline bool ks_finite(float x) { return fabsf(x) < INFINITY; }   // false on NaN

// order-preserving map float -> uint32 (finite values), and back
__device__ inline uint32_t ks_enc(float x) {
    const uint32_t b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ inline float ks_dec(uint32_t u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// bmin[d], bmax[d] = min, max of the finite coordinates, encoded; the caller set bmin = ~0, bmax = 0
__global__ __launch_bounds__(256) void k_ks_bbox(const float* __restrict__ x, int64_t n, int D,
                                                 uint32_t* __restrict__ bmin, uint32_t* __restrict__ bmax) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    for (int d = 0; d < D; ++d) {
        const float v = i < n ? x[i * D + d] : NAN;
        const bool fin = ks_finite(v);
        uint32_t lo = fin ? ks_enc(v) : 0xffffffffu, hi = fin ? ks_enc(v) : 0u;
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const uint32_t ol = __shfl_xor(lo, s), oh = __shfl_xor(hi, s);
            lo = ol < lo ? ol : lo;
            hi = oh > hi ? oh : hi;
        }
        if (lane == 0) {
            if (lo != 0xffffffffu) atomicMin(bmin + d, lo);
            if (hi != 0u) atomicMax(bmax + d, hi);
        }
    }
}

// Morton key of every row inside the union of the points' and the queries' box; val = the row
__global__ __launch_bounds__(256) void k_ks_keys(const float* __restrict__ x, int64_t n, int D,
                                                 const uint32_t* __restrict__ box, int with_query_box,
                                                 uint64_t* __restrict__ key, int32_t* __restrict__ val) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int bits = 63 / D < 21 ? 63 / D : 21;
    const float cells = (float)(1u << bits);
    uint32_t cell[kKsDMax];
    bool ok = true;
#pragma unroll
    for (int d = 0; d < kKsDMax; ++d) {
        cell[d] = 0;
        if (d >= D) continue;
        uint32_t ulo = box[d], uhi = box[2 * kKsDMax + d];
        if (with_query_box) {
            const uint32_t ql = box[kKsDMax + d], qh = box[3 * kKsDMax + d];
            ulo = ql < ulo ? ql : ulo;
            uhi = qh > uhi ? qh : uhi;
        }
        const float lo = ks_dec(ulo), hi = ks_dec(uhi), v = x[i * D + d];
        ok = ok && ks_finite(v);
        const float ext = hi - lo;
        const float scale = (ext > 0.f && ext < INFINITY) ? cells / ext : 0.f;   // degenerate box: every cell 0
        float c = (v - lo) * scale;
        c = c > 0.f ? c : 0.f;                                                   // NaN -> 0
        c = c < cells - 1.f ? c : cells - 1.f;
        cell[d] = (uint32_t)c;
    }
    uint64_t k = 0;
    if (ok) {
        for (int b = bits - 1; b >= 0; --b)
#pragma unroll
            for (int d = 0; d < kKsDMax; ++d)
                if (d < D) k = (k << 1) | ((cell[d] >> b) & 1u);
    } else {
        k = kKsKeyNonFinite;
    }
    key[i] = k;
    val[i] = (int32_t)i;
}

// one workgroup per tile of 256 sorted rows: the zero-padded sorted copy, the tile's box over the finite
// coordinates (padding dimensions 0) and its non-finite flag
template <int DP>
__global__ __launch_bounds__(256) void k_ks_gather(const float* __restrict__ points, int64_t np, int D,
                                                   const int32_t* __restrict__ perm, float* __restrict__ spts,
                                                   float* __restrict__ tlo, float* __restrict__ thi,
                                                   int32_t* __restrict__ tflag) {
    __shared__ float s_lo[kLkWaves][DP], s_hi[kLkWaves][DP];
    __shared__ int s_bad[kLkWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * kLkTile + threadIdx.x;
    const bool act = row < np;
    const int64_t src = act ? perm[row] : 0;
    bool bad = false;
#pragma unroll
    for (int d = 0; d < DP; ++d) {
        const float v = (act && d < D) ? points[src * D + d] : 0.f;
        if (act) spts[row * DP + d] = v;
        const bool fin = ks_finite(v);
        bad = bad || !fin;
        float lo = (act && fin) ? v : INFINITY, hi = (act && fin) ? v : -INFINITY;
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, s));
            hi = fmaxf(hi, __shfl_xor(hi, s));
        }
        if (lane == 0) {
            s_lo[wave][d] = lo;
            s_hi[wave][d] = hi;
        }
    }
    const uint64_t any_bad = __ballot(bad);
    if (lane == 0) s_bad[wave] = any_bad != 0;
    __syncthreads();
    if (threadIdx.x < DP) {
        const int d = threadIdx.x;
        float lo = s_lo[0][d], hi = s_hi[0][d];
        for (int w = 1; w < kLkWaves; ++w) {
            lo = fminf(lo, s_lo[w][d]);
            hi = fmaxf(hi, s_hi[w][d]);
        }
        tlo[(int64_t)blockIdx.x * DP + d] = lo;
        thi[(int64_t)blockIdx.x * DP + d] = hi;
    }
    if (threadIdx.x == 0) tflag[blockIdx.x] = s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3];
}

template <int DP>
__global__ __launch_bounds__(kLkWaves * 64) void k_knn_sorted(
    const float* __restrict__ query, int64_t nq, const int32_t* __restrict__ qperm,
    const uint64_t* __restrict__ qkey_s, const float* __restrict__ spts, const int32_t* __restrict__ pperm,
    const uint64_t* __restrict__ pkey_s, int64_t np, int D, int K, float radius, const float* __restrict__ r_dev,
    const float* __restrict__ tlo, const float* __restrict__ thi, const int32_t* __restrict__ tflag,
    int64_t* __restrict__ idx_out, float* __restrict__ d2_out, int32_t* __restrict__ wg_stats) {
    __shared__ __attribute__((aligned(16))) float tile[kLkTile * DP];
    __shared__ int32_t tperm[kLkTile];
    __shared__ uint64_t bufs[kLkWaves][kLkQ][kLkCap];
    __shared__ int s_skip[2][kLkWaves];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t g0 = (int64_t)blockIdx.x * kKsGroup;
    const int64_t q0 = g0 + wave * kLkQ;
    const float rr = r_dev != nullptr ? *r_dev : radius;
    const float r2 = rr * rr;
    const int64_t T = (np + kLkTile - 1) / kLkTile;
    float qv[kLkQ][DP];
    float thr[kLkQ];
    int cnt[kLkQ];
    int64_t row[kLkQ];
    float wlo[DP], whi[DP];
#pragma unroll
    for (int d = 0; d < DP; ++d) {
        wlo[d] = INFINITY;
        whi[d] = -INFINITY;
    }
    bool wave_live = false;
#pragma unroll
    for (int j = 0; j < kLkQ; ++j) {
        const bool act = q0 + j < nq;
        row[j] = act ? (int64_t)qperm[q0 + j] : -1;
        bool live = act;
#pragma unroll
        for (int d = 0; d < DP; ++d) {
            qv[j][d] = (act && d < D) ? query[row[j] * D + d] : 0.f;
            live = live && ks_finite(qv[j][d]);
        }
        // a query with a non-finite coordinate has d2 = inf or NaN for every point: it takes nothing, as absent ones
        thr[j] = live ? 3.0e38f : -1.f;
        cnt[j] = 0;
        if (live) {
            wave_live = true;
#pragma unroll
            for (int d = 0; d < DP; ++d) {
                wlo[d] = fminf(wlo[d], qv[j][d]);
                whi[d] = fmaxf(whi[d], qv[j][d]);
            }
        }
    }
    // home tile: the last tile whose first key is <= the key of the group's first query
    int64_t home = 0;
    {
        const uint64_t k = qkey_s[g0];
        int64_t lo = 0, hi = T;   // first tile with first key > k
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (pkey_s[mid * kLkTile] <= k) lo = mid + 1;
            else hi = mid;
        }
        home = lo > 0 ? lo - 1 : 0;
    }
    int64_t up = home, dn = home - 1;
    bool turn_up = true;
    int visited = 0, skipped = 0;
    for (int64_t it = 0; it < T; ++it) {
        int64_t t;
        if ((turn_up && up < T) || dn < 0) t = up++;
        else t = dn--;
        if (it > 0) turn_up = !turn_up;   // home, home + 1, home - 1, home + 2, ...
        bool skip_w = !wave_live;
        if (wave_live) {
            float lb = 0.f;
#pragma unroll
            for (int d = 0; d < DP; ++d) {
                const float a = tlo[t * DP + d] - whi[d], b = wlo[d] - thi[t * DP + d];
                float g = a > 0.f ? a : 0.f;
                g = b > g ? b : g;
                lb = fmaf(g, g, lb);
            }
            float bound = -1.f;
#pragma unroll
            for (int j = 0; j < kLkQ; ++j) {
                const float b = thr[j] < r2 ? thr[j] : r2;
                bound = b > bound ? b : bound;
            }
            skip_w = tflag[t] == 0 && r2 == r2 && lb >= kKsLbMin && lb < INFINITY && lb * kKsSlack > bound;
        }
        if (lane == 0) s_skip[it & 1][wave] = skip_w;
        __syncthreads();   // the flags of this tile are written; every wave has left the previous tile
        if (s_skip[it & 1][0] && s_skip[it & 1][1] && s_skip[it & 1][2] && s_skip[it & 1][3]) {
            ++skipped;
            continue;
        }
        ++visited;
        const int64_t base = t * kLkTile;
        const int n = (np - base) < kLkTile ? (int)(np - base) : kLkTile;
        {
            const lk_f32x4* src = (const lk_f32x4*)(spts + base * DP);
            lk_f32x4* dst = (lk_f32x4*)tile;
            for (int i = threadIdx.x; i < n * (DP / 4); i += kLkWaves * 64) dst[i] = src[i];
            if ((int)threadIdx.x < n) tperm[threadIdx.x] = pperm[base + threadIdx.x];
        }
        __syncthreads();
        if (skip_w) continue;
        for (int c0 = 0; c0 < n; c0 += 64) {
            const int c = c0 + lane;
            const bool valid = c < n;
            float pv[DP];
#pragma unroll
            for (int v = 0; v < DP / 4; ++v) {
                const lk_f32x4 p4 = *(const lk_f32x4*)(tile + (valid ? c : 0) * DP + v * 4);
                pv[v * 4 + 0] = p4.x;
                pv[v * 4 + 1] = p4.y;
                pv[v * 4 + 2] = p4.z;
                pv[v * 4 + 3] = p4.w;
            }
            float d2q[kLkQ];
#pragma unroll
            for (int j = 0; j < kLkQ; ++j) {
                float d2 = 0.f;
#pragma unroll
                for (int d = 0; d < DP; ++d) {
                    const float t_ = qv[j][d] - pv[d];
                    d2 = fmaf(t_, t_, d2);
                }
                d2q[j] = d2;
            }
            const int idx = tperm[valid ? c : 0];
#pragma unroll
            for (int j = 0; j < kLkQ; ++j) {
                const bool pass = valid && d2q[j] < r2 && d2q[j] <= thr[j];
                const uint64_t m = __ballot(pass);
                if (m == 0) continue;
                uint64_t* buf = bufs[wave][j];
                if (cnt[j] + 64 > kLkCap) {
                    cnt[j] = lk_flush(buf, cnt[j], K, lane, &thr[j]);
                    lk_wave_sync();
                }
                const int below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
                if (pass) buf[cnt[j] + below] = lk_key(d2q[j], idx);
                cnt[j] += __popcll(m);
            }
        }
    }
    if (threadIdx.x == 0) {
        wg_stats[2 * (int64_t)blockIdx.x] = visited;
        wg_stats[2 * (int64_t)blockIdx.x + 1] = skipped;
    }
#pragma unroll
    for (int j = 0; j < kLkQ; ++j) {
        if (row[j] < 0) continue;
        uint64_t* buf = bufs[wave][j];
        float unused;
        const int c = lk_flush(buf, cnt[j], K, lane, &unused);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = lane * 4 + i;
            if (e >= K) continue;
            const bool ok = e < c;
            const uint64_t key = ok ? buf[e] : kLkEmpty;
            idx_out[row[j] * K + e] = ok ? (int64_t)(uint32_t)key : (int64_t)-1;
            if (d2_out != nullptr) d2_out[row[j] * K + e] = ok ? __uint_as_float((uint32_t)(key >> 32)) : -1.f;
        }
    }
}

// the workgroups' counters summed in a fixed order (thread-strided partial sums, then a tree over the threads)
__global__ __launch_bounds__(256) void k_ks_stats(const int32_t* __restrict__ wg, int64_t groups,
                                                  int64_t* __restrict__ ws_stats, int64_t* __restrict__ stats_out) {
    __shared__ int64_t s[2][256];
    int64_t v = 0, k = 0;
    for (int64_t g = threadIdx.x; g < groups; g += 256) {
        v += wg[2 * g];
        k += wg[2 * g + 1];
    }
    s[0][threadIdx.x] = v;
    s[1][threadIdx.x] = k;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            s[0][threadIdx.x] += s[0][threadIdx.x + w];
            s[1][threadIdx.x] += s[1][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x < 2) {
        ws_stats[threadIdx.x] = s[threadIdx.x][0];
        if (stats_out != nullptr) stats_out[threadIdx.x] = s[threadIdx.x][0];
    }
}

// np == 0: every slot is padding
__global__ __launch_bounds__(256) void k_ks_fill(int64_t n, int64_t* __restrict__ idx_out,
                                                 float* __restrict__ d2_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    idx_out[i] = -1;
    if (d2_out != nullptr) d2_out[i] = -1.f;
}

unsigned ks_blocks(int64_t n) { return (unsigned)ceil_div(n > 0 ? n : 1, 256); }

int ks_check(const char* who, int64_t nq, int64_t np, int32_t D, int32_t K) {
    HGNN_REQUIRE(nq >= 0 && np >= 0 && np < ((int64_t)1 << 31) && nq < ((int64_t)1 << 31), "%s: bad sizes", who);
    HGNN_REQUIRE(D >= 1 && D <= kKsDMax, "%s: D must be in [1, %d] (got %d)", who, kKsDMax, D);
    HGNN_REQUIRE(K >= 1 && K <= kLkKMax, "%s: K must be in [1, %d] (got %d)", who, kLkKMax, K);
    return HGNN_OK;
}

}  // namespace
}  // namespace hgnn

using namespace hgnn;

extern "C" int hgnn_knn_sorted_workspace_bytes(int64_t nq, int64_t np, int32_t D, int32_t K, size_t* bytes) {
    const char* who = "hgnn_knn_sorted_workspace_bytes";
    int rc = ks_check(who, nq, np, D, K);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE(bytes != nullptr, "%s: NULL bytes", who);
    KsWorkspace w;
    rc = ks_layout(nq, np, ks_dp(D), &w, nullptr);
    if (rc != HGNN_OK) return rc;
    *bytes = w.total;
    return HGNN_OK;
}

extern "C" int hgnn_knn_radius_sorted_f32(const float* query, int64_t nq, const float* points, int64_t np, int32_t D,
                                          int32_t K, float radius, const float* radius_dev, int64_t* idx_out,
                                          float* dist2_out, void* workspace, size_t workspace_bytes,
                                          int64_t* stats_out, hgnn_stream_t stream_) {
    const char* who = "hgnn_knn_radius_sorted_f32";
    hipStream_t stream = (hipStream_t)stream_;
    int rc = ks_check(who, nq, np, D, K);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE(radius_dev != nullptr || radius >= 0.f, "%s: negative radius", who);
    if (nq == 0) return HGNN_OK;
    HGNN_REQUIRE(query != nullptr && idx_out != nullptr && (np == 0 || points != nullptr), "%s: NULL pointer", who);
    const int DP = ks_dp(D);
    KsWorkspace w;
    rc = ks_layout(nq, np, DP, &w, stream);
    if (rc != HGNN_OK) return rc;
    if (workspace == nullptr || workspace_bytes < w.total || (uintptr_t)workspace % 16 != 0) {
        set_error("%s: workspace too small (%zu < %zu) or unaligned", who, workspace_bytes, w.total);
        return HGNN_ERR_WORKSPACE;
    }
    char* ws = (char*)workspace;
    int64_t* stats = (int64_t*)(ws + w.stats);
    if (np == 0) {
        k_ks_fill<<<ks_blocks(nq * K), 256, 0, stream>>>(nq * K, idx_out, dist2_out);
        HGNN_CHECK_HIP(hipMemsetAsync(stats, 0, 2 * sizeof(int64_t), stream));
        if (stats_out != nullptr) HGNN_CHECK_HIP(hipMemsetAsync(stats_out, 0, 2 * sizeof(int64_t), stream));
        HGNN_CHECK_HIP(hipGetLastError());
        return HGNN_OK;
    }
    uint32_t* box = (uint32_t*)(ws + w.box);
    int32_t* wg = (int32_t*)(ws + w.wg);
    uint64_t *pkey = (uint64_t*)(ws + w.pkey), *pkey_s = (uint64_t*)(ws + w.pkey_s);
    int32_t *pval = (int32_t*)(ws + w.pval), *pperm = (int32_t*)(ws + w.pperm);
    uint64_t *qkey = (uint64_t*)(ws + w.qkey), *qkey_s = (uint64_t*)(ws + w.qkey_s);
    int32_t *qval = (int32_t*)(ws + w.qval), *qperm = (int32_t*)(ws + w.qperm);
    float *spts = (float*)(ws + w.spts), *tlo = (float*)(ws + w.tlo), *thi = (float*)(ws + w.thi);
    int32_t* tflag = (int32_t*)(ws + w.tflag);
    void* temp = ws + w.temp;
    size_t tb = w.temp_bytes;
    const bool shared = query == points && nq == np;   // frnn_graph: one sort serves both sides

    // box = {pmin[16], qmin[16], pmax[16], qmax[16]}: the empty box is min = ~0, max = 0
    HGNN_CHECK_HIP(hipMemsetAsync(box, 0xff, 2 * kKsDMax * 4, stream));
    HGNN_CHECK_HIP(hipMemsetAsync(box + 2 * kKsDMax, 0, 2 * kKsDMax * 4, stream));
    k_ks_bbox<<<ks_blocks(np), 256, 0, stream>>>(points, np, D, box, box + 2 * kKsDMax);
    if (!shared) k_ks_bbox<<<ks_blocks(nq), 256, 0, stream>>>(query, nq, D, box + kKsDMax, box + 3 * kKsDMax);
    k_ks_keys<<<ks_blocks(np), 256, 0, stream>>>(points, np, D, box, shared ? 0 : 1, pkey, pval);
    HGNN_CHECK_HIP(rocprim::radix_sort_pairs(temp, tb, pkey, pkey_s, pval, pperm, (size_t)np, 0u, 64u, stream));
    if (!shared) {
        k_ks_keys<<<ks_blocks(nq), 256, 0, stream>>>(query, nq, D, box, 1, qkey, qval);
        HGNN_CHECK_HIP(rocprim::radix_sort_pairs(temp, tb, qkey, qkey_s, qval, qperm, (size_t)nq, 0u, 64u, stream));
    } else {
        qkey_s = pkey_s;
        qperm = pperm;
    }
    const unsigned tiles = (unsigned)ceil_div(np, kLkTile), groups = (unsigned)ceil_div(nq, kKsGroup);
#define HGNN_KS_DP(DPV)                                                                                             \
    do {                                                                                                            \
        k_ks_gather<DPV><<<tiles, 256, 0, stream>>>(points, np, D, pperm, spts, tlo, thi, tflag);                   \
        k_knn_sorted<DPV><<<groups, kLkWaves * 64, 0, stream>>>(query, nq, qperm, qkey_s, spts, pperm, pkey_s, np,  \
                                                                D, K, radius, radius_dev, tlo, thi, tflag, idx_out, \
                                                                dist2_out, wg);                                     \
    } while (0)
    if (DP == 4) HGNN_KS_DP(4);
    else if (DP == 8) HGNN_KS_DP(8);
    else HGNN_KS_DP(16);
#undef HGNN_KS_DP
    k_ks_stats<<<1, 256, 0, stream>>>(wg, (int64_t)groups, stats, stats_out);
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}
