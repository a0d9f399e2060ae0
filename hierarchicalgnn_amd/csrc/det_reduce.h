// The deterministic float64 reduction of the scalar-result operators: k_ph_* (pairloss.hip), k_wb_* (wbce.hip),
// k_opt_* (optim.hip) and k_ga_* (graphcon.hip).  "Two calls return the same bits" rests on three things, all owned
// by this file:
//   1. the grid is a function of the problem size alone (det_grid; never of the device, a tuning option or the load),
//   2. every workgroup reduces its 256 per-thread sums through ONE fixed tree (block_sum) and writes ONE partial per
//      accumulator at partials[k * gridDim.x + blockIdx.x] (write_partials),
//   3. a single workgroup adds the partials in index order -- thread t takes t, t + 256, .. -- and then goes through
//      the same tree (total_partials).
// The per-thread order before step 2 (which elements a thread adds, and in which order) is the kernel's own and is a
// function of the grid, hence of the size.
#pragma once
#include "common.h"
#include <type_traits>

namespace hgnn {

// ---------------------------------------------------------------------------------------------------- device side
// fixed-shape sum of one double per thread over the workgroup: xor tree inside the wave, then the waves in order.
// The tree is fixed, so the result is a function of the 256 inputs only; lds holds kWavesPerBlock doubles; every
// thread of the workgroup must call it (it synchronises), and every thread gets the sum.
static __device__ __forceinline__ double block_sum(double v, double* lds) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    const int wave = threadIdx.x / kWave;
    __syncthreads();
    if (threadIdx.x % kWave == 0) lds[wave] = v;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < kWavesPerBlock; ++w) t += lds[w];
    return t;
}

// one partial per workgroup and accumulator.  The layout partials[k * gridDim.x + blockIdx.x] is part of the contract:
// total_partials reads it with n_partials = the grid of the kernel that wrote it, and the kernels that keep these two
// loops written out (their code would change otherwise) use the same layout.
template <int NACC>
static __device__ __forceinline__ void write_partials(const double* acc, double* lds, double* __restrict__ partials) {
    for (int k = 0; k < NACC; ++k) {
        const double s = block_sum(acc[k], lds);
        if (threadIdx.x == 0) partials[(int64_t)k * gridDim.x + blockIdx.x] = s;
    }
}

// thread t adds partials t, t + 256, .. in that order, then the fixed tree (one workgroup)
template <int NACC>
static __device__ __forceinline__ void total_partials(const double* __restrict__ partials, int n_partials, double* lds,
                                                      double* tot) {
    for (int k = 0; k < NACC; ++k) {
        double v = 0.0;
        for (int j = threadIdx.x; j < n_partials; j += kBlock) v += partials[(int64_t)k * n_partials + j];
        tot[k] = block_sum(v, lds);
    }
}

// the ids of VEC = 16 / sizeof(IT) consecutive pairs as one 16-byte load per endpoint row
template <class IT>
struct alignas(16) PairIds {
    IT v[16 / sizeof(IT)];
};

template <class IT, bool VEC_OK>
static __device__ __forceinline__ void load_pair_ids(const IT* __restrict__ row, int64_t first, int n, int64_t* out) {
    constexpr int VEC = 16 / sizeof(IT);
    if (VEC_OK && n == VEC) {
        const PairIds<IT> t = *reinterpret_cast<const PairIds<IT>*>(row + first);
#pragma unroll
        for (int j = 0; j < VEC; ++j) out[j] = (int64_t)t.v[j];
    } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) out[j] = j < n ? (int64_t)row[first + j] : 0;
    }
}

// ------------------------------------------------------------------------------------------------------ host side
constexpr int kDetMaxGrid = 2048;   // 256 CUs x 8 workgroups: cap, then grid-stride; also the most partials per sum

// the grid of a kernel with `threads` units of work, one per thread and trip: a function of that number alone
static inline unsigned det_grid(int64_t threads) {
    const int64_t blocks = ceil_div(threads, kBlock);
    return (unsigned)(blocks < 1 ? 1 : (blocks > kDetMaxGrid ? kDetMaxGrid : blocks));
}

// fn(index type tag, VEC_OK): the two compile-time choices of a kernel that reads the [2, P] id rows of `graph`
// through load_pair_ids.  VEC_OK: both rows can be read as 16-byte words.
template <class Fn>
static inline void with_index_type(int32_t index_dtype, const void* graph, int64_t P, Fn&& fn) {
    const size_t isz = index_dtype == HGNN_DT_I64 ? 8 : 4;
    const bool vec_ok = (uintptr_t)graph % 16 == 0 && ((size_t)P * isz) % 16 == 0;
    auto with_vec = [&](auto it) {
        if (vec_ok) fn(it, std::true_type{});
        else fn(it, std::false_type{});
    };
    if (index_dtype == HGNN_DT_I64) with_vec((int64_t)0);
    else with_vec((int32_t)0);
}

}  // namespace hgnn
