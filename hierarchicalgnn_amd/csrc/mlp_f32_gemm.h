// The fp32-MFMA GEMM step shared by the fused fp32 forward (mlp_fused.hip) and the fp32 backward layer
// (mlp_bwd_f32.hip): weight chunks staged through LDS in A-fragment order, v_mfma_f32_16x16x4_f32 on tile pairs.
#pragma once
#include "mlp_common.h"

namespace hgnn {

template <int NF, int NW>
__device__ __forceinline__ void stage_w(const float* __restrict__ W, int Kdim, int k0, float* lds,
                                        int wave, int lane) {
    WStage st = begin_stage<NW>(W, Kdim, k0, lds, wave, lane);
    const int n = pieces_of<NF, NW>(wave);
    for (int i = 0; i < n; ++i) stage_next<NW>(st);
}

// One k-chunk (16 k-values) of one layer:  acc[T] += Wchunk[T] * b  for every 16-feature tile T.
// Tiles are processed in pairs (two independent accumulators cover the 40-cycle dependent-issue
// latency of v_mfma_f32_16x16x4_f32) and the NEXT pair's weight fragments are fetched from LDS
// before the current pair's 8 MFMAs, pinned with sched_group_barrier so that hipcc does not
// sink the reads back to their first use.  The LDS-DMA pieces that stage the NEXT chunk's weights
// are issued one at a time BETWEEN MFMA groups (each costs the issuing wave ~60 cycles of VMEM
// issue; in a burst ahead of the loop they were 10 % of the kernel, in the MFMA shadow they hide).
template <int NT, int NF_NEXT, int NW>
__device__ __forceinline__ void mma_chunk(f32x4 (&acc)[NT], const float* __restrict__ wb, const f32x4 b,
                                          WStage& st, int n_pieces) {
    static_assert(NT % 2 == 0, "tiles are processed in pairs");
    constexpr int PAIRS = NT / 2;
    constexpr int PER_WAVE = (NF_NEXT / 16 + NW - 1) / NW;
    constexpr int EVERY = PAIRS >= PER_WAVE ? PAIRS / PER_WAVE : 1;
    f32x4 w0 = *(const f32x4*)(wb);
    f32x4 w1 = *(const f32x4*)(wb + 256);
    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);  // pipeline prologue: the first pair's reads
    int issued = 0;
#pragma unroll
    for (int T = 0; T < NT; T += 2) {
        f32x4 n0 = w0, n1 = w1;
        if (T + 2 < NT) {
            n0 = *(const f32x4*)(wb + (T + 2) * 256);
            n1 = *(const f32x4*)(wb + (T + 3) * 256);
        }
        if (((T / 2) % EVERY == 0) && issued < PER_WAVE) {
            if (__builtin_amdgcn_readfirstlane(issued < n_pieces ? 1 : 0)) stage_next<NW>(st);  // scalar branch
            ++issued;
        }
        acc[T] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.x, b.x, acc[T], 0, 0, 0);
        acc[T + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.x, b.x, acc[T + 1], 0, 0, 0);
        acc[T] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.y, b.y, acc[T], 0, 0, 0);
        acc[T + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.y, b.y, acc[T + 1], 0, 0, 0);
        acc[T] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.z, b.z, acc[T], 0, 0, 0);
        acc[T + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.z, b.z, acc[T + 1], 0, 0, 0);
        acc[T] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.w, b.w, acc[T], 0, 0, 0);
        acc[T + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.w, b.w, acc[T + 1], 0, 0, 0);
        w0 = n0;
        w1 = n1;
        if (T + 2 < NT) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);  // 2 DS reads (next pair)
        __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);                  // 8 MFMAs (this pair)
    }
    for (int i = issued; i < n_pieces; ++i) stage_next<NW>(st);  // more pieces than tile pairs
}

}  // namespace hgnn
