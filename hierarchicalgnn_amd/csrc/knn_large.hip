// Fixed-radius kNN for 33 <= K <= 128 (the embedding stage's FRNN_graph, knn: 100 in
// GNNEmbedding/Configs/*.yaml).  K <= 32 stays on k_knn_radius / k_knn_merge (knn.hip).
//
// The register list of k_knn_radius does not scale to K = 100 (2K VGPRs per lane, and every insertion
// walks the whole list).  Here the lanes of a wave run over the CANDIDATES instead:
//   * a wave owns kLkQ queries; their coordinates are wave-uniform;
//   * point tiles are staged in LDS and shared by the workgroup's four waves;
//   * a candidate with d2 < r2 and d2 <= thr_q is appended to query q's LDS buffer (kLkCap entries; the slot
//     comes from a ballot prefix count);
//   * when a buffer cannot take another 64 entries, the wave sorts it by the key (d2, idx) -- a bitonic sort
//     of kLkCap = 256 entries in registers, 4 per lane -- keeps the first K and sets thr_q to the K-th d2;
//   * a final sort writes the K rows.
// Entries are compared as the 64-bit key (float bits of d2) << 32 | idx: d2 >= 0, so the float bits order
// like the floats, and the key order is the lexicographic (d2, idx) order.  The selected set is therefore
// the K smallest keys whatever the lane order, the tiling or the candidate split: the result does not depend
// on the algorithm, and its first 32 columns equal the K = 32 kernel's bit for bit.
//
// d2 is k_knn_radius's arithmetic: zero-padded DP, t = q - p, d2 = fmaf(t, t, d2) in dimension order;
// r2 = r * r in float32.  No global atomics.
//
// SPLIT (few queries): blockIdx.y selects a slice of the candidates, each slice writes its sorted K keys to
// the workspace, and k_knn_large_merge selects the K smallest keys of all slices (exact, as above).
#include "common.h"
#include "knn_select.h"

namespace hgnn {

template <int DP, bool SPLIT>
__global__ __launch_bounds__(kLkWaves * 64) void k_knn_large(const float* __restrict__ query, int64_t nq,
                                                             const float* __restrict__ points, int64_t np_all, int D,
                                                             int K, float radius, const float* __restrict__ r_dev,
                                                             int64_t* __restrict__ idx_out, float* __restrict__ d2_out,
                                                             int64_t slice_len, uint64_t* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float tile[kLkTile * DP];
    __shared__ uint64_t bufs[kLkWaves][kLkQ][kLkCap];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t q0 = ((int64_t)blockIdx.x * kLkWaves + wave) * kLkQ;
    const float rr = r_dev != nullptr ? *r_dev : radius;
    const float r2 = rr * rr;
    const int64_t p_begin = SPLIT ? (int64_t)blockIdx.y * slice_len : 0;
    const int64_t np = SPLIT ? ((p_begin + slice_len) < np_all ? (p_begin + slice_len) : np_all) : np_all;
    float qv[kLkQ][DP];
    float thr[kLkQ];
    int cnt[kLkQ];
#pragma unroll
    for (int j = 0; j < kLkQ; ++j) {
        const bool act = q0 + j < nq;
#pragma unroll
        for (int d = 0; d < DP; ++d) qv[j][d] = (act && d < D) ? query[(q0 + j) * D + d] : 0.f;
        thr[j] = act ? 3.0e38f : -1.f;   // an absent query takes nothing
        cnt[j] = 0;
    }
    for (int64_t base = p_begin; base < np; base += kLkTile) {
        const int n = (np - base) < kLkTile ? (int)(np - base) : kLkTile;
        __syncthreads();
        for (int t = threadIdx.x; t < n * DP; t += kLkWaves * 64) {
            const int pt = t / DP, d = t % DP;
            tile[t] = d < D ? points[(base + pt) * D + d] : 0.f;
        }
        __syncthreads();
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
                    const float t = qv[j][d] - pv[d];
                    d2 = fmaf(t, t, d2);
                }
                d2q[j] = d2;
            }
            const int idx = (int)(base + c);
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
#pragma unroll
    for (int j = 0; j < kLkQ; ++j) {
        const int64_t q = q0 + j;
        if (q >= nq) continue;
        uint64_t* buf = bufs[wave][j];
        float unused;
        const int c = lk_flush(buf, cnt[j], K, lane, &unused);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = lane * 4 + i;
            if (e >= K) continue;
            const uint64_t key = e < c ? buf[e] : kLkEmpty;
            if constexpr (SPLIT) {
                part[((size_t)q * gridDim.y + blockIdx.y) * K + e] = key;
            } else {
                const bool ok = e < c;
                idx_out[q * K + e] = ok ? (int64_t)(uint32_t)key : (int64_t)-1;
                if (d2_out != nullptr) d2_out[q * K + e] = ok ? __uint_as_float((uint32_t)(key >> 32)) : -1.f;
            }
        }
    }
}

// one wave per query: the K smallest keys over the slices' sorted lists (positions [0, 128) keep the running
// selection, positions [128, 256) take the next slice)
__global__ __launch_bounds__(256) void k_knn_large_merge(int64_t nq, int slices, int K,
                                                         const uint64_t* __restrict__ part,
                                                         int64_t* __restrict__ idx_out, float* __restrict__ d2_out) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;
    uint64_t k[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) k[i] = kLkEmpty;
    for (int s = 0; s < slices; ++s) {
        const uint64_t* src = part + ((size_t)q * slices + s) * K;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = lane * 4 + i - kLkKMax;
            if (e >= 0) k[i] = e < K ? src[e] : kLkEmpty;
        }
        lk_sort256(k, lane);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = lane * 4 + i;
        if (e >= K) continue;
        const bool ok = k[i] != kLkEmpty;
        idx_out[q * K + e] = ok ? (int64_t)(uint32_t)k[i] : (int64_t)-1;
        if (d2_out != nullptr) d2_out[q * K + e] = ok ? __uint_as_float((uint32_t)(k[i] >> 32)) : -1.f;
    }
}

}  // namespace hgnn

using namespace hgnn;

// candidate slices for the large-K kernel: enough workgroups to fill the chip, whole tiles per slice
void hgnn_knn_large_slices(int64_t nq, int64_t np, int* slices, int64_t* slice_len) {
    *slices = 1;
    *slice_len = np;
    const int64_t blocks = ceil_div(nq, kLkWaves * kLkQ);
    if (blocks >= 1024 || np < 2 * kLkTile) return;
    int64_t want = ceil_div((int64_t)2048, blocks > 0 ? blocks : 1);
    if (want > 32) want = 32;
    if (want <= 1) return;
    const int64_t len = ceil_div(ceil_div(np, want), (int64_t)kLkTile) * kLkTile;
    *slice_len = len;
    *slices = (int)ceil_div(np, len);
}

// 33 <= K <= 128 (arguments checked by the caller, knn_dispatch); ws == NULL: no split
int hgnn_knn_large_launch(const float* query, int64_t nq, const float* points, int64_t np, int D, int K, float radius,
                          const float* r_dev, int64_t* idx_out, float* d2_out, void* ws, hipStream_t stream) {
    int slices;
    int64_t slice_len;
    hgnn_knn_large_slices(nq, np, &slices, &slice_len);
    if (ws == nullptr) {
        slices = 1;
        slice_len = np;
    }
    const bool split = slices > 1;
    uint64_t* part = (uint64_t*)ws;
    const dim3 grid((unsigned)ceil_div(nq, kLkWaves * kLkQ), (unsigned)slices);
#define HGNN_LK_DP(DP)                                                                                          \
    do {                                                                                                        \
        if (split)                                                                                              \
            k_knn_large<DP, true><<<grid, kLkWaves * 64, 0, stream>>>(query, nq, points, np, D, K, radius, r_dev, \
                                                                      idx_out, d2_out, slice_len, part);        \
        else                                                                                                    \
            k_knn_large<DP, false><<<grid, kLkWaves * 64, 0, stream>>>(query, nq, points, np, D, K, radius,       \
                                                                       r_dev, idx_out, d2_out, np, nullptr);    \
    } while (0)
    if (D <= 4) HGNN_LK_DP(4);
    else if (D <= 8) HGNN_LK_DP(8);
    else HGNN_LK_DP(16);
#undef HGNN_LK_DP
    if (split)
        k_knn_large_merge<<<(unsigned)ceil_div(nq, 4), 256, 0, stream>>>(nq, slices, K, part, idx_out, d2_out);
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}
