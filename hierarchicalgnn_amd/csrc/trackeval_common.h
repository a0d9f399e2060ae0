// What hgnn_track_eval (trackeval.hip) and hgnn_track_records (trackeval_records.hip) share: the workspace layout,
// the run / contingency kernels, the per-particle kernels and the fixed-order reduction.  The data flow and the
// numerics are described at the top of trackeval.hip.  Everything lives in an unnamed namespace: each of the two
// translation units gets its own copy, and each includes this file after `#pragma clang fp contract(off)`.
#pragma once
#include "common.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#pragma clang fp contract(off)

namespace hgnn {
namespace {

constexpr int kRedBlocks = 256;   // first level of the final reduction
constexpr int kMaxWaveBlocks = 2048;

struct TeWorkspace {
    // candidate stage [B]
    size_t cv_in, cv, ck, cflag, crid, cstart, ckeep, kscan, ccol;
    // contingency stage [B]
    size_t key, skey, tflag, trid, tstart;
    // particle stage [N]
    size_t pv_in, pv, pk, pflag, prid, pstart, hit_p, nhits, opid, ptmin, prim, prow_b, prow_e;
    size_t pp_sum, pp_cnt;
    // reduction and status
    size_t blk_sum, blk_cnt, err;
    size_t temp, temp_bytes, total;
};

inline int bit_width(int64_t x) {  // smallest b >= 1 with 2^b > x
    int b = 1;
    while (b < 62 && ((int64_t)1 << b) <= x) ++b;
    return b;
}

inline int te_layout(int64_t B, int64_t N, TeWorkspace* w, hipStream_t stream) {
    const unsigned key_end = (unsigned)(bit_width(N) + bit_width(B));
    size_t t1 = 0, t2 = 0, t3 = 0, t4 = 0, t5 = 0;
    if (B > 0) {
        HGNN_CHECK_HIP(rocprim::radix_sort_pairs(nullptr, t1, (int64_t*)nullptr, (int64_t*)nullptr,
                                                 (int32_t*)nullptr, (int32_t*)nullptr, (size_t)B, 0u, 64u,
                                                 stream));
        HGNN_CHECK_HIP(rocprim::radix_sort_keys(nullptr, t2, (uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)B,
                                                0u, key_end, stream));
        HGNN_CHECK_HIP(rocprim::inclusive_scan(nullptr, t3, (int32_t*)nullptr, (int32_t*)nullptr, (size_t)B,
                                               rocprim::plus<int32_t>(), stream));
    }
    if (N > 0) {
        HGNN_CHECK_HIP(rocprim::radix_sort_pairs(nullptr, t4, (int64_t*)nullptr, (int64_t*)nullptr,
                                                 (int32_t*)nullptr, (int32_t*)nullptr, (size_t)N, 0u, 64u,
                                                 stream));
        HGNN_CHECK_HIP(rocprim::inclusive_scan(nullptr, t5, (int32_t*)nullptr, (int32_t*)nullptr, (size_t)N,
                                               rocprim::plus<int32_t>(), stream));
    }
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    };
    const size_t b = (size_t)B, n = (size_t)N;
    w->cv_in = take(b * 4);
    w->cv = take(b * 4);
    w->ck = take(b * 8);
    w->cflag = take(b * 4);
    w->crid = take(b * 4);
    w->cstart = take((b + 1) * 4);
    w->ckeep = take(b * 4);
    w->kscan = take(b * 4);
    w->ccol = take(b * 4);
    w->key = take(b * 8);
    w->skey = take(b * 8);
    w->tflag = take(b * 4);
    w->trid = take(b * 4);
    w->tstart = take((b + 1) * 4);
    w->pv_in = take(n * 4);
    w->pv = take(n * 4);
    w->pk = take(n * 8);
    w->pflag = take(n * 4);
    w->prid = take(n * 4);
    w->pstart = take((n + 1) * 4);
    w->hit_p = take(n * 4);
    w->nhits = take(n * 4);
    w->opid = take(n * 8);
    w->ptmin = take(n * 4);
    w->prim = take(n * 4);
    w->prow_b = take(n * 4);
    w->prow_e = take(n * 4);
    w->pp_sum = take(n * 2 * sizeof(double));
    w->pp_cnt = take(n * sizeof(int4));
    w->blk_sum = take(kRedBlocks * 2 * sizeof(double));
    w->blk_cnt = take(kRedBlocks * 4 * sizeof(long long));
    w->err = take(sizeof(int32_t));
    size_t t = t1;
    for (size_t x : {t2, t3, t4, t5}) t = x > t ? x : t;
    w->temp_bytes = t;
    w->temp = take(t + 256);
    w->total = off;
    return HGNN_OK;
}

__global__ __launch_bounds__(256) void k_te_iota(int32_t* __restrict__ v, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = i;
}

// run heads of sorted keys; with Limited, positions with key >= limit (the sentinel tail) belong to no run
template <typename K, bool Limited>
__device__ inline bool in_run(K k, K limit) { return !Limited || k < limit; }

template <typename K, bool Limited>
__global__ __launch_bounds__(256) void k_te_heads(const K* __restrict__ keys, int n, K limit,
                                                  int32_t* __restrict__ flag) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    K k = keys[i];
    flag[i] = (in_run<K, Limited>(k, limit) && (i == 0 || k != keys[i - 1])) ? 1 : 0;
}

// start[r] = first position of run r (rid = inclusive scan of the heads, 1-based); start[R] = end of the last run
template <typename K, bool Limited>
__global__ __launch_bounds__(256) void k_te_starts(const K* __restrict__ keys, const int32_t* __restrict__ flag,
                                                   const int32_t* __restrict__ rid, int n, K limit,
                                                   int32_t* __restrict__ start) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (flag[i]) start[rid[i] - 1] = i;
    if (in_run<K, Limited>(keys[i], limit) && (i == n - 1 || !in_run<K, Limited>(keys[i + 1], limit)))
        start[rid[i]] = i + 1;
}

// step 1: size filter over the candidate runs (slot r < B; runs r >= R are absent)
__global__ __launch_bounds__(256) void k_te_cand_keep(const int32_t* __restrict__ cstart,
                                                      const int32_t* __restrict__ crid, int B, float thr,
                                                      int32_t* __restrict__ keep) {
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= B) return;
    const int R = crid[B - 1];
    // torch: int64 count >= Python float runs in float32 (default dtype promotion)
    keep[r] = (r < R && (float)(cstart[r + 1] - cstart[r]) >= thr) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_te_hit_particle(const int32_t* __restrict__ pv,
                                                         const int32_t* __restrict__ prid, int N,
                                                         int32_t* __restrict__ hit_p) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) hit_p[pv[i]] = prid[i] - 1;
}

// the contingency key of every pair, walked in candidate-sorted order
__global__ __launch_bounds__(256) void k_te_pair_keys(const int32_t* __restrict__ cv, const int32_t* __restrict__ crid,
                                                      const int32_t* __restrict__ cstart,
                                                      const int32_t* __restrict__ keep,
                                                      const int32_t* __restrict__ kscan,
                                                      const int64_t* __restrict__ hit,
                                                      const int32_t* __restrict__ hit_p, int B, int N, int cbits,
                                                      uint64_t* __restrict__ key, int32_t* __restrict__ ccol,
                                                      int32_t* __restrict__ err) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const int r = crid[i] - 1;
    const bool kept = keep[r] != 0;
    const int c = kscan[r] - 1;
    const int64_t h = hit[cv[i]];
    const bool bad = h < 0 || h >= N;
    if (bad) atomicOr(err, 1);
    uint64_t k = (uint64_t)N << cbits;  // sentinel: sorts after every valid key
    if (kept && !bad) k = ((uint64_t)hit_p[h] << cbits) | (uint64_t)c;
    key[i] = k;
    if (kept && i == cstart[r]) ccol[c] = cstart[r + 1] - cstart[r];
}

// row range [prow_b, prow_e) of every particle in the triple list (rows without a triple stay [0, 0))
__global__ __launch_bounds__(256) void k_te_rows(const uint64_t* __restrict__ skey,
                                                 const int32_t* __restrict__ tstart,
                                                 const int32_t* __restrict__ trid, int B, int cbits,
                                                 int32_t* __restrict__ prow_b, int32_t* __restrict__ prow_e) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int M = trid[B - 1];
    if (t >= M) return;
    const int p = (int)(skey[tstart[t]] >> cbits);
    if (t == 0 || (int)(skey[tstart[t - 1]] >> cbits) != p) prow_b[p] = t;
    if (t == M - 1 || (int)(skey[tstart[t + 1]] >> cbits) != p) prow_e[p] = t + 1;
}

__device__ inline double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ inline int wave_isum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ inline double wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// the minimum in which a NaN wins (torch amin): once m is NaN neither test holds again
__device__ inline float nan_min(float m, float v) { return (v < m || v != v) ? v : m; }
__device__ inline float wave_nan_min(float m) {
    for (int o = 32; o > 0; o >>= 1) m = nan_min(m, __shfl_xor(m, o));  // a NaN in any lane reaches every lane
    return m;
}

// step 2: one wave per particle over its hits (in ascending hit order: the sort is stable).  ptmin is the minimum
// with NaN propagation: a particle with a NaN pt has ptmin = NaN, fails `ptmin > pt_cut` and is not reconstructable
__global__ __launch_bounds__(256) void k_te_particles(const int32_t* __restrict__ pstart,
                                                      const int32_t* __restrict__ prid,
                                                      const int32_t* __restrict__ pv, const int64_t* __restrict__ pk,
                                                      const float* __restrict__ pt,
                                                      const uint8_t* __restrict__ primary, int N,
                                                      int32_t* __restrict__ nhits, int64_t* __restrict__ opid,
                                                      float* __restrict__ ptmin, int32_t* __restrict__ prim) {
    const int lane = threadIdx.x & 63;
    const int P = prid[N - 1];
    for (int p = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; p < P; p += (gridDim.x * blockDim.x) >> 6) {
        const int b = pstart[p], e = pstart[p + 1];
        float m = __builtin_inff();
        int any = 0;
        for (int j = b + lane; j < e; j += 64) {
            const int h = pv[j];
            m = nan_min(m, pt[h]);
            if (primary != nullptr && primary[h] != 0) any = 1;
        }
        m = wave_nan_min(m);
        any = wave_isum(any);
        if (lane == 0) {
            nhits[p] = e - b;
            opid[p] = pk[b];
            ptmin[p] = m;
            prim[p] = any > 0;
        }
    }
}

__device__ inline double hash_of(int c, int C, double step) {
    constexpr double stop = 1.0 + 1e-12;
    if (C == 1) return 1.0;
    if (c == C - 1) return stop;
    const double t = (double)c * step;  // rounded: this file is compiled with contraction off
    return t + 1.0;
}

struct TeParams {
    double majority_cut, nhits_cut, keep_cut;  // keep_cut = majority_cut * nhits_cut
    float pt_cut;
    int use_primary;
};

// what k_te_match<true> stores beyond the scalar path (hgnn_track_records); k_te_match<false> takes the empty form
// and does no store of it
template <bool Records>
struct TeMatchRecords {};
template <>
struct TeMatchRecords<true> {
    int32_t* cand_index;            // [P] smallest c among the particle's kept matches, or -1
    int32_t* shared;                // [P] that triple's n, or 0
    int32_t* masked_hits;           // [P] sum of n over the particle's masked triples
    int32_t* c_kept;                // [C] kept matches of the candidate (integer atomics; zeroed before)
    int32_t* c_mask;                // [C] masked matches
    unsigned long long* c_first;    // [C] min of p << 32 | n over the kept matches (all ones before)
};

// steps 3-7 per particle (one wave): matches among the particle's triples, and the particle's share of every sum
template <bool Records>
__global__ __launch_bounds__(256) void k_te_match(const int32_t* __restrict__ prow_b, const int32_t* __restrict__ prow_e,
                                                  const uint64_t* __restrict__ skey,
                                                  const int32_t* __restrict__ tstart,
                                                  const int32_t* __restrict__ ccol, const int32_t* __restrict__ kscan,
                                                  const int32_t* __restrict__ prid, const int32_t* __restrict__ nhits,
                                                  const int64_t* __restrict__ opid, const float* __restrict__ ptmin,
                                                  const int32_t* __restrict__ prim, int B, int N, int cbits,
                                                  TeParams prm, double* __restrict__ pp_sum,
                                                  int4* __restrict__ pp_cnt, TeMatchRecords<Records> rec) {
    constexpr double delta = (1.0 + 1e-12) - 1.0;
    const int lane = threadIdx.x & 63;
    const int P = prid[N - 1];
    const int C = kscan[B - 1];
    const double step = C > 1 ? delta / (double)(C - 1) : 0.0;
    const uint64_t cmask = ((uint64_t)1 << cbits) - 1;
    for (int p = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; p < P; p += (gridDim.x * blockDim.x) >> 6) {
        const int b = prow_b[p], e = prow_e[p];
        const double nh_p = (double)nhits[p];
        const bool prim_ok = !prm.use_primary || prim[p] != 0;
        const bool recon = ptmin[p] > prm.pt_cut && nh_p >= prm.nhits_cut && prim_ok;
        const bool noise = opid[p] == 0;
        double rmax = 0.0;
        for (int t = b + lane; t < e; t += 64) {
            const double n = (double)(tstart[t + 1] - tstart[t]);
            const int c = (int)(skey[tstart[t]] & cmask);
            rmax = fmax(rmax, n * hash_of(c, C, step));
        }
        rmax = wave_max(rmax);
        double hp = 0.0, he = 0.0;
        int n_match = 0, n_kept = 0, n_mask = 0;
        unsigned long long first = ~0ull;   // Records: min of c << 32 | n over the kept matches
        int masked_hits = 0;
        for (int t = b + lane; t < e; t += 64) {
            const int ni = tstart[t + 1] - tstart[t];
            const double n = (double)ni;
            const int c = (int)(skey[tstart[t]] & cmask);
            const double col = (double)ccol[c];
            const bool match = n >= prm.majority_cut * col && n >= nh_p * prm.majority_cut &&
                               n * hash_of(c, C, step) == rmax;
            const bool kept = match && n > prm.keep_cut && !noise;
            const bool mask = kept && recon;
            n_match += match;
            n_kept += kept;
            n_mask += mask;
            if (kept) hp += n / col;
            if (mask) he += n / nh_p;
            if constexpr (Records) {
                if (kept) {
                    const unsigned long long mine = ((unsigned long long)(unsigned)c << 32) | (unsigned)ni;
                    first = mine < first ? mine : first;
                    atomicAdd(&rec.c_kept[c], 1);
                    atomicMin(&rec.c_first[c], ((unsigned long long)(unsigned)p << 32) | (unsigned)ni);
                }
                if (mask) {
                    masked_hits += ni;
                    atomicAdd(&rec.c_mask[c], 1);
                }
            }
        }
        hp = wave_sum(hp);
        he = wave_sum(he);
        n_match = wave_isum(n_match);
        n_kept = wave_isum(n_kept);
        n_mask = wave_isum(n_mask);
        if constexpr (Records) {
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long other = __shfl_xor(first, o);
                first = other < first ? other : first;
            }
            masked_hits = wave_isum(masked_hits);
        }
        if (lane == 0) {
            pp_sum[2 * p] = hp;
            pp_sum[2 * p + 1] = he;
            pp_cnt[p] = make_int4(n_match, n_kept, n_mask, recon ? 1 : 0);
            if constexpr (Records) {
                const bool any = first != ~0ull;
                rec.cand_index[p] = any ? (int32_t)(first >> 32) : -1;
                rec.shared[p] = any ? (int32_t)(first & 0xffffffffu) : 0;
                rec.masked_hits[p] = masked_hits;
            }
        }
    }
}

// first level of the final reduction: block k sums particles [k * chunk, (k + 1) * chunk) in a fixed order
__global__ __launch_bounds__(256) void k_te_reduce(const double* __restrict__ pp_sum, const int4* __restrict__ pp_cnt,
                                                   const int32_t* __restrict__ prid, int N,
                                                   double* __restrict__ blk_sum, long long* __restrict__ blk_cnt) {
    __shared__ double s_sum[2][256];
    __shared__ long long s_cnt[4][256];
    const int P = prid[N - 1];
    const int chunk = (P + kRedBlocks - 1) / kRedBlocks;
    const int lo = blockIdx.x * chunk, hi = min(P, lo + chunk);
    double a = 0.0, bsum = 0.0;
    long long c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (int p = lo + (int)threadIdx.x; p < hi; p += 256) {
        a += pp_sum[2 * p];
        bsum += pp_sum[2 * p + 1];
        const int4 c = pp_cnt[p];
        c0 += c.x;
        c1 += c.y;
        c2 += c.z;
        c3 += c.w;
    }
    const int tid = threadIdx.x;
    s_sum[0][tid] = a;
    s_sum[1][tid] = bsum;
    s_cnt[0][tid] = c0;
    s_cnt[1][tid] = c1;
    s_cnt[2][tid] = c2;
    s_cnt[3][tid] = c3;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            for (int k = 0; k < 2; ++k) s_sum[k][tid] += s_sum[k][tid + s];
            for (int k = 0; k < 4; ++k) s_cnt[k][tid] += s_cnt[k][tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        blk_sum[2 * blockIdx.x] = s_sum[0][0];
        blk_sum[2 * blockIdx.x + 1] = s_sum[1][0];
        for (int k = 0; k < 4; ++k) blk_cnt[4 * blockIdx.x + k] = s_cnt[k][0];
    }
}

// second level (one block of kRedBlocks threads) and the metrics.  run: the pipeline ran (there were pairs and hits);
// without it the row is the default response with P still counted.  status: what HGNN_TE_STATUS receives
__device__ inline void te_finalize_row(const double* __restrict__ blk_sum, const long long* __restrict__ blk_cnt,
                                       const int32_t* __restrict__ prid, const int32_t* __restrict__ kscan, int B, int N,
                                       bool run, double status, double* __restrict__ result) {
    __shared__ double s_sum[2][kRedBlocks];
    __shared__ long long s_cnt[4][kRedBlocks];
    const int tid = threadIdx.x;
    for (int k = 0; k < 2; ++k) s_sum[k][tid] = run ? blk_sum[2 * tid + k] : 0.0;
    for (int k = 0; k < 4; ++k) s_cnt[k][tid] = run ? blk_cnt[4 * tid + k] : 0;
    __syncthreads();
    for (int s = kRedBlocks / 2; s > 0; s >>= 1) {
        if (tid < s) {
            for (int k = 0; k < 2; ++k) s_sum[k][tid] += s_sum[k][tid + s];
            for (int k = 0; k < 4; ++k) s_cnt[k][tid] += s_cnt[k][tid + s];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const long long C = run ? kscan[B - 1] : 0;
    const long long P = N > 0 ? prid[N - 1] : 0;
    const long long n_match = s_cnt[0][0], n_kept = s_cnt[1][0], n_mask = s_cnt[2][0], n_truth = s_cnt[3][0];
    // numpy true division of integer sums: 0/0 = nan, x/0 = inf
    result[HGNN_TE_TRACK_EFF] = (double)n_mask / (double)n_truth;
    result[HGNN_TE_TRACK_PUR] = (double)n_mask / (double)(C - (n_match - n_kept) - (n_kept - n_mask));
    result[HGNN_TE_HIT_EFF] = s_sum[1][0] / (double)n_mask;
    result[HGNN_TE_HIT_PUR] = s_sum[0][0] / (double)n_kept;
    result[HGNN_TE_N_KEPT] = (double)n_kept;
    result[HGNN_TE_N_MASK] = (double)n_mask;
    result[HGNN_TE_N_TRUTH] = (double)n_truth;
    result[HGNN_TE_N_CAND] = (double)C;
    result[HGNN_TE_N_PART] = (double)P;
    result[HGNN_TE_NO_MATCH] = (n_match == 0 || n_kept == 0) ? 1.0 : 0.0;
    result[HGNN_TE_STATUS] = status;
    result[HGNN_TE_N_MATCH] = (double)n_match;
}

__global__ __launch_bounds__(kRedBlocks) void k_te_finalize(const double* __restrict__ blk_sum,
                                                            const long long* __restrict__ blk_cnt,
                                                            const int32_t* __restrict__ prid,
                                                            const int32_t* __restrict__ kscan, int B, int N,
                                                            const int32_t* __restrict__ err,
                                                            double* __restrict__ result) {
    const bool run = B > 0 && N > 0;
    te_finalize_row(blk_sum, blk_cnt, prid, kscan, B, N, run, (run && *err != 0) ? 1.0 : 0.0, result);
}

inline unsigned blocks_for(int64_t n) { return (unsigned)ceil_div(n > 0 ? n : 1, 256); }
inline unsigned wave_blocks(int64_t n) {  // one wave per item, 4 waves per block, grid-stride beyond the cap
    int64_t b = ceil_div(n > 0 ? n : 1, kWavesPerBlock);
    return (unsigned)(b < kMaxWaveBlocks ? b : kMaxWaveBlocks);
}

inline int te_check_sizes(const char* who, int64_t n_pairs, int64_t n_hits) {
    HGNN_REQUIRE(n_pairs >= 0 && n_hits >= 0, "%s: negative size", who);
    HGNN_REQUIRE(n_pairs < ((int64_t)1 << 31) - 1 && n_hits < ((int64_t)1 << 31) - 1,
                 "%s: more than 2^31 - 2 pairs or hits", who);
    return HGNN_OK;
}

// ---------------------------------------------------------------------------------------------- launch sequences
// The pipeline in stages, so that a caller that evaluates many pair sets of ONE event (trackscan.hip) runs the
// particle stage once.  hgnn_track_eval is te_candidate_runs, k_te_cand_keep + te_candidate_relabel,
// te_particle_stage, te_match_stage and k_te_finalize, in that order.
struct TePtrs {
    int32_t *cv_in, *cv, *cflag, *crid, *cstart, *ckeep, *kscan, *ccol;
    int64_t* ck;
    uint64_t *key, *skey;
    int32_t *tflag, *trid, *tstart;
    int32_t *pv_in, *pv, *pflag, *prid, *pstart, *hit_p, *nhits, *prim, *prow_b, *prow_e, *err;
    int64_t *pk, *opid;
    float* ptmin;
    double *pp_sum, *blk_sum;
    int4* pp_cnt;
    long long* blk_cnt;
    void* temp;
    size_t temp_bytes;
};

inline TePtrs te_ptrs(void* workspace, const TeWorkspace& w) {
    char* ws = (char*)workspace;
    auto I32 = [&](size_t o) { return (int32_t*)(ws + o); };
    TePtrs p;
    p.cv_in = I32(w.cv_in), p.cv = I32(w.cv), p.cflag = I32(w.cflag), p.crid = I32(w.crid);
    p.cstart = I32(w.cstart), p.ckeep = I32(w.ckeep), p.kscan = I32(w.kscan), p.ccol = I32(w.ccol);
    p.ck = (int64_t*)(ws + w.ck);
    p.key = (uint64_t*)(ws + w.key), p.skey = (uint64_t*)(ws + w.skey);
    p.tflag = I32(w.tflag), p.trid = I32(w.trid), p.tstart = I32(w.tstart);
    p.pv_in = I32(w.pv_in), p.pv = I32(w.pv), p.pflag = I32(w.pflag), p.prid = I32(w.prid);
    p.pstart = I32(w.pstart), p.hit_p = I32(w.hit_p), p.nhits = I32(w.nhits), p.prim = I32(w.prim);
    p.prow_b = I32(w.prow_b), p.prow_e = I32(w.prow_e), p.err = I32(w.err);
    p.pk = (int64_t*)(ws + w.pk), p.opid = (int64_t*)(ws + w.opid);
    p.ptmin = (float*)(ws + w.ptmin);
    p.pp_sum = (double*)(ws + w.pp_sum), p.blk_sum = (double*)(ws + w.blk_sum);
    p.pp_cnt = (int4*)(ws + w.pp_cnt);
    p.blk_cnt = (long long*)(ws + w.blk_cnt);
    p.temp = ws + w.temp;
    p.temp_bytes = w.temp_bytes;
    return p;
}

// the status word and the row ranges of one evaluation
inline int te_clear(const TePtrs& p, int N, hipStream_t stream) {
    HGNN_CHECK_HIP(hipMemsetAsync(p.err, 0, sizeof(int32_t), stream));
    HGNN_CHECK_HIP(hipMemsetAsync(p.prow_b, 0, (size_t)N * 4, stream));
    HGNN_CHECK_HIP(hipMemsetAsync(p.prow_e, 0, (size_t)N * 4, stream));
    return HGNN_OK;
}

// step 1 up to the size filter: the runs of equal candidate labels (B > 0)
inline int te_candidate_runs(const TePtrs& p, const int64_t* cand, int B, hipStream_t stream) {
    size_t tb = p.temp_bytes;
    k_te_iota<<<blocks_for(B), 256, 0, stream>>>(p.cv_in, B);
    HGNN_CHECK_HIP(rocprim::radix_sort_pairs(p.temp, tb, cand, p.ck, p.cv_in, p.cv, (size_t)B, 0u, 64u, stream));
    k_te_heads<int64_t, false><<<blocks_for(B), 256, 0, stream>>>(p.ck, B, 0, p.cflag);
    HGNN_CHECK_HIP(rocprim::inclusive_scan(p.temp, tb, p.cflag, p.crid, (size_t)B, rocprim::plus<int32_t>(), stream));
    k_te_starts<int64_t, false><<<blocks_for(B), 256, 0, stream>>>(p.ck, p.cflag, p.crid, B, 0, p.cstart);
    return HGNN_OK;
}

// step 1 after the size filter: the dense label of every kept run
inline int te_candidate_relabel(const TePtrs& p, int B, hipStream_t stream) {
    size_t tb = p.temp_bytes;
    HGNN_CHECK_HIP(rocprim::inclusive_scan(p.temp, tb, p.ckeep, p.kscan, (size_t)B, rocprim::plus<int32_t>(), stream));
    return HGNN_OK;
}

// step 2: the particles (N > 0).  Nothing here depends on the pairs
inline int te_particle_stage(const TePtrs& p, const int64_t* pid, const float* pt, const uint8_t* primary, int N,
                             hipStream_t stream) {
    size_t tb = p.temp_bytes;
    k_te_iota<<<blocks_for(N), 256, 0, stream>>>(p.pv_in, N);
    HGNN_CHECK_HIP(rocprim::radix_sort_pairs(p.temp, tb, pid, p.pk, p.pv_in, p.pv, (size_t)N, 0u, 64u, stream));
    k_te_heads<int64_t, false><<<blocks_for(N), 256, 0, stream>>>(p.pk, N, 0, p.pflag);
    HGNN_CHECK_HIP(rocprim::inclusive_scan(p.temp, tb, p.pflag, p.prid, (size_t)N, rocprim::plus<int32_t>(), stream));
    k_te_starts<int64_t, false><<<blocks_for(N), 256, 0, stream>>>(p.pk, p.pflag, p.prid, N, 0, p.pstart);
    k_te_hit_particle<<<blocks_for(N), 256, 0, stream>>>(p.pv, p.prid, N, p.hit_p);
    k_te_particles<<<wave_blocks(N), 256, 0, stream>>>(p.pstart, p.prid, p.pv, p.pk, pt, primary, N, p.nhits, p.opid,
                                                       p.ptmin, p.prim);
    return HGNN_OK;
}

// steps 3-7 up to the first level of the reduction (B > 0, N > 0): contingency triples, matching, block sums
inline int te_match_stage(const TePtrs& p, const int64_t* hit, int B, int N, const TeParams& prm,
                          hipStream_t stream) {
    size_t tb = p.temp_bytes;
    const int cbits = bit_width(B), pbits = bit_width(N);
    const uint64_t sentinel = (uint64_t)N << cbits;
    k_te_pair_keys<<<blocks_for(B), 256, 0, stream>>>(p.cv, p.crid, p.cstart, p.ckeep, p.kscan, hit, p.hit_p, B, N,
                                                      cbits, p.key, p.ccol, p.err);
    HGNN_CHECK_HIP(rocprim::radix_sort_keys(p.temp, tb, p.key, p.skey, (size_t)B, 0u, (unsigned)(pbits + cbits),
                                            stream));
    k_te_heads<uint64_t, true><<<blocks_for(B), 256, 0, stream>>>(p.skey, B, sentinel, p.tflag);
    HGNN_CHECK_HIP(rocprim::inclusive_scan(p.temp, tb, p.tflag, p.trid, (size_t)B, rocprim::plus<int32_t>(), stream));
    k_te_starts<uint64_t, true><<<blocks_for(B), 256, 0, stream>>>(p.skey, p.tflag, p.trid, B, sentinel, p.tstart);
    k_te_rows<<<blocks_for(B), 256, 0, stream>>>(p.skey, p.tstart, p.trid, B, cbits, p.prow_b, p.prow_e);
    k_te_match<false><<<wave_blocks(N), 256, 0, stream>>>(p.prow_b, p.prow_e, p.skey, p.tstart, p.ccol, p.kscan,
                                                          p.prid, p.nhits, p.opid, p.ptmin, p.prim, B, N, cbits, prm,
                                                          p.pp_sum, p.pp_cnt, TeMatchRecords<false>{});
    k_te_reduce<<<kRedBlocks, 256, 0, stream>>>(p.pp_sum, p.pp_cnt, p.prid, N, p.blk_sum, p.blk_cnt);
    return HGNN_OK;
}

}  // namespace
}  // namespace hgnn
