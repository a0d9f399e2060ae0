// The selection helpers of the large-K kNN kernels (knn_large.hip, knn_sorted.hip): a wave keeps a query's
// candidates as 64-bit keys (float bits of d2) << 32 | idx in an LDS buffer of kLkCap entries and cuts it to the K
// smallest with a bitonic sort in registers.  d2 >= 0, so the float bits order like the floats and the key order is
// the lexicographic (d2, idx) order.
#pragma once
#include "common.h"

namespace hgnn {

constexpr int kLkQ = 4;        // queries per wave
constexpr int kLkWaves = 4;    // waves per workgroup
constexpr int kLkTile = 256;   // candidate points per LDS tile
constexpr int kLkCap = 256;    // buffer entries per query (>= 128 kept + 64 appended)
constexpr int kLkKMax = 128;
constexpr uint64_t kLkEmpty = ~(uint64_t)0;

typedef float lk_f32x4 __attribute__((ext_vector_type(4)));

// order of LDS accesses of one wave across its lanes (LDS executes one wave's operations in order; this keeps
// the compiler from moving them across the point)
__device__ inline void lk_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ inline uint64_t lk_key(float d2, int idx) {
    return ((uint64_t)__float_as_uint(d2) << 32) | (uint32_t)idx;
}

// ascending bitonic sort of the 256 keys held 4 per lane, element e = lane * 4 + i
__device__ inline void lk_sort256(uint64_t (&k)[4], int lane) {
#pragma unroll
    for (int size = 2; size <= kLkCap; size <<= 1) {
#pragma unroll
        for (int j = size >> 1; j > 0; j >>= 1) {
            if (j >= 4) {
                const int lj = j >> 2;
                const bool lower = (lane & lj) == 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const uint64_t o = __shfl_xor(k[i], lj);
                    const bool asc = ((lane * 4 + i) & size) == 0;
                    const bool take_min = asc == lower;
                    const uint64_t mn = k[i] < o ? k[i] : o, mx = k[i] < o ? o : k[i];
                    k[i] = take_min ? mn : mx;
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (i & j) continue;
                    const bool asc = ((lane * 4 + i) & size) == 0;
                    const uint64_t a = k[i], b = k[i | j];
                    const bool swap = asc ? (b < a) : (a < b);
                    k[i] = swap ? b : a;
                    k[i | j] = swap ? a : b;
                }
            }
        }
    }
}

// the key at sorted position p (wave-uniform p)
__device__ inline uint64_t lk_at(const uint64_t (&k)[4], int p) {
    const int i = p & 3;
    const uint64_t v = i == 0 ? k[0] : i == 1 ? k[1] : i == 2 ? k[2] : k[3];
    return __shfl(v, p >> 2);
}

// sort query buffer `buf` (cnt valid entries), keep the K smallest at its front; returns the new count and sets
// thr to the K-th distance once K entries exist
__device__ inline int lk_flush(uint64_t* buf, int cnt, int K, int lane, float* thr) {
    lk_wave_sync();
    uint64_t k[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) k[i] = (lane * 4 + i) < cnt ? buf[lane * 4 + i] : kLkEmpty;
    lk_sort256(k, lane);
    lk_wave_sync();
#pragma unroll
    for (int i = 0; i < 4; ++i) buf[lane * 4 + i] = k[i];
    lk_wave_sync();
    if (cnt >= K) {
        *thr = __uint_as_float((uint32_t)(lk_at(k, K - 1) >> 32));
        return K;
    }
    return cnt;
}

}  // namespace hgnn
