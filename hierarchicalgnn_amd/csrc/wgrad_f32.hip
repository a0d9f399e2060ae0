// Weight gradient of one Linear layer of the EXACT fp32 training path, hand-written for the fp32 MFMA:
//
//     dW[ho][hi] = sum_m dz[m][ho] * a[m][hi]            dz: [M, Ho] fp32,  a: [M, Hi] fp32,  dW: fp32
//
// (backward of Modules/utils.py:169-196's Linear layers as used by the edge / node networks,
// Modules/gnn_utils.py:22-41).  The same "TN" GEMM as wgrad_bf16.hip -- the reduction runs over the rows, the result
// is tiny -- with every product formed ONCE from the fp32 operands by v_mfma_f32_16x16x4_f32: no split, no
// reduced-precision plane.  Per output element the instruction is a k-ordered fmaf chain, so a slice's partial is
//     acc = fmaf(dz[m][ho], a[m][hi], acc)   for m = first row of the slice .. its last, in order,
// and the result is the partials added in slice order by k_wgrad_f32_reduce (four chains, fixed order).  No atomics;
// slices, rows per slice and tile are a pure function of (M, Ho, Hi) (wgf::shape_for): the same inputs give the same
// bits on every device and in every run.
//   * the 16x16x4 form wants, per lane, A[i = l & 15][k = l >> 4] = dz[m0 + k][ho0 + i] and
//     B[k = l >> 4][j = l & 15] = a[m0 + k][hi0 + j]: both operands are read ALONG the rows as they lie in memory, a
//     16-lane group takes 16 consecutive floats of row m0 + k.  The tiles are stored row-major in LDS as they arrive
//     ([KT m][T columns], 16 B per lane) and read back with plain ds_read_b32 -- no transposing load;
//   * LDS row stride = T + 16 words (== 16 mod 32): the 4 rows x 16 words of one fragment read fall on distinct banks;
//   * D[ho][hi] accumulates in registers over the whole slice (128 fp32 per lane for the 128 x 64 wave tile of the
//     256 x 256 workgroup tile), written once as a partial [S][Ho][Hi].
#include "common.h"

namespace hgnn {
namespace wgf {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// rows of m per step = four v_mfma_f32_16x16x4_f32 along k.  32 rows per step, and reading the fragments of k group
// kk + 1 into a second register set while the MFMAs of group kk issue, both measured within +-2 % of this form
constexpr int KT = 16;

// TO x TI output tile per workgroup, WO x WI waves, each wave (TO/WO) x (TI/WI)
template <int TO, int TI, int WO, int WI>
__global__ __launch_bounds__(WO * WI * 64) void k_wgrad_f32(const float* __restrict__ A, long long lda,
                                                            const float* __restrict__ B, long long ldb, long long M,
                                                            int Ho, int Hi, float* __restrict__ partial,
                                                            long long rows_per_slice) {
    constexpr int NTHR = WO * WI * 64;
    constexpr int SA = TO + 16, SB = TI + 16;          // LDS row strides in floats
    constexpr int PA = TO / 4, PB = TI / 4;            // 16-byte pieces per tile row
    constexpr int NPA = KT * PA / NTHR, NPB = KT * PB / NTHR;
    static_assert(KT * PA % NTHR == 0 && KT * PB % NTHR == 0, "tile pieces must divide over the threads");
    constexpr int FO = TO / WO / 16, FI = TI / WI / 16;
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    float* As = smem_f;
    float* Bs = smem_f + 2 * KT * SA;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wo = wave % WO, wi = wave / WO;
    const int n_to = (Ho + TO - 1) / TO;
    const int ho0 = (int)(blockIdx.x % n_to) * TO;
    const int hi0 = (int)(blockIdx.x / n_to) * TI;
    const long long m_begin = (long long)blockIdx.y * rows_per_slice;
    long long m_end = m_begin + rows_per_slice;
    if (m_end > M) m_end = M;
    const int steps = m_end > m_begin ? (int)((m_end - m_begin + KT - 1) / KT) : 0;

    f32x4 ra[NPA], rb[NPB];
    auto load = [&](int s) {   // rows past the slice and columns past the matrix arrive as zeros: fmaf(0, 0, acc) = acc
        const long long m0 = m_begin + (long long)s * KT;
        const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < NPA; ++i) {
            const int idx = tid + i * NTHR;
            const int row = idx / PA, col = ho0 + (idx % PA) * 4;
            ra[i] = (m0 + row < m_end && col < Ho) ? *(const f32x4*)(A + (size_t)(m0 + row) * (size_t)lda + col) : z4;
        }
#pragma unroll
        for (int i = 0; i < NPB; ++i) {
            const int idx = tid + i * NTHR;
            const int row = idx / PB, col = hi0 + (idx % PB) * 4;
            rb[i] = (m0 + row < m_end && col < Hi) ? *(const f32x4*)(B + (size_t)(m0 + row) * (size_t)ldb + col) : z4;
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NPA; ++i) {
            const int idx = tid + i * NTHR;
            *(f32x4*)(As + buf * KT * SA + (idx / PA) * SA + (idx % PA) * 4) = ra[i];
        }
#pragma unroll
        for (int i = 0; i < NPB; ++i) {
            const int idx = tid + i * NTHR;
            *(f32x4*)(Bs + buf * KT * SB + (idx / PB) * SB + (idx % PB) * 4) = rb[i];
        }
    };

    f32x4 acc[FO][FI];
#pragma unroll
    for (int fo = 0; fo < FO; ++fo)
#pragma unroll
        for (int fi = 0; fi < FI; ++fi) acc[fo][fi] = f32x4{0.f, 0.f, 0.f, 0.f};

    if (steps > 0) {
        load(0);
        store(0);
    }
    __syncthreads();
    // fragment element of this lane: row (lane >> 4) of a 4-row k group, column (lane & 15) of a 16-column block
    const int frag_a = (lane >> 4) * SA + wo * (TO / WO) + (lane & 15);
    const int frag_b = (lane >> 4) * SB + wi * (TI / WI) + (lane & 15);
    for (int s = 0; s < steps; ++s) {   // `steps` is uniform over the workgroup: every wave takes every barrier
        const bool more = s + 1 < steps;
        if (more) load(s + 1);
        const float* at = As + (s & 1) * KT * SA + frag_a;
        const float* bt = Bs + (s & 1) * KT * SB + frag_b;
#pragma unroll
        for (int kk = 0; kk < KT / 4; ++kk) {   // rows m0 + 4 kk .. + 3: the k order of the chain is the row order
            float a[FO], b[FI];
#pragma unroll
            for (int fi = 0; fi < FI; ++fi) b[fi] = bt[4 * kk * SB + fi * 16];
#pragma unroll
            for (int fo = 0; fo < FO; ++fo) a[fo] = at[4 * kk * SA + fo * 16];
            // consecutive MFMAs write different accumulators (dependent latency 40 cycles against a 32-cycle issue)
#pragma unroll
            for (int fo = 0; fo < FO; ++fo)
#pragma unroll
                for (int fi = 0; fi < FI; ++fi)
                    acc[fo][fi] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[fo], b[fi], acc[fo][fi], 0, 0, 0);
        }
        if (more) store((s + 1) & 1);
        __syncthreads();
    }
    // D layout: column (hi) = lane & 15, rows (ho) = 4 * (lane >> 4) + r
    float* out = partial + (size_t)blockIdx.y * (size_t)Ho * (size_t)Hi;
#pragma unroll
    for (int fo = 0; fo < FO; ++fo) {
#pragma unroll
        for (int fi = 0; fi < FI; ++fi) {
            const int hi = hi0 + wi * (TI / WI) + fi * 16 + (lane & 15);
            const int ho = ho0 + wo * (TO / WO) + fo * 16 + 4 * (lane >> 4);
            if (hi < Hi) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (ho + r < Ho) out[(size_t)(ho + r) * (size_t)Hi + hi] = acc[fo][fi][r];
            }
        }
    }
}

// the S partials in slice order: the four-chain order of wg::k_wgrad_reduce (wgrad_bf16.hip), without its column sums
__global__ __launch_bounds__(256) void k_wgrad_f32_reduce(const float* __restrict__ partial, int slices, int Ho, int Hi,
                                                          float* __restrict__ out, long long ldo) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long n = (long long)Ho * Hi;
    if (i >= n) return;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int k = 0;
    for (; k + 3 < slices; k += 4) {
        s0 += partial[(size_t)k * (size_t)n + i];
        s1 += partial[(size_t)(k + 1) * (size_t)n + i];
        s2 += partial[(size_t)(k + 2) * (size_t)n + i];
        s3 += partial[(size_t)(k + 3) * (size_t)n + i];
    }
    for (; k < slices; ++k) s0 += partial[(size_t)k * (size_t)n + i];
    out[(size_t)(i / Hi) * (size_t)ldo + (i % Hi)] = (s0 + s1) + (s2 + s3);
}

struct Shape {
    int to, ti, tiles, slices;
    long long rows_per_slice;
};

// a pure function of (M, Ho, Hi): never of the device (tests/wgrad_f32_ref.py restates it)
static Shape shape_for(long long M, int Ho, int Hi) {
    Shape s;
    s.to = Ho > 128 ? 256 : 128;
    s.ti = (Ho > 128 && Hi > 128) ? 256 : 128;   // larger tiles = fewer re-reads of the rows
    s.tiles = (int)(ceil_div(Ho, s.to) * ceil_div(Hi, s.ti));
    // ~512 workgroups in total; every slice costs a [Ho, Hi] fp32 partial that the reduce pass reads back
    long long want = ceil_div((long long)512, s.tiles);
    long long max_slices = ceil_div(M, (long long)KT * 8);   // at least 8 steps per slice
    if (want > max_slices) want = max_slices;
    if (want < 1) want = 1;
    s.rows_per_slice = ceil_div(ceil_div(M, want), (long long)KT) * KT;
    if (s.rows_per_slice < KT) s.rows_per_slice = KT;
    s.slices = (int)ceil_div(M > 0 ? M : 1, s.rows_per_slice);
    return s;
}

static bool widths_ok(int Ho, int Hi) {
    return Ho > 0 && Hi > 0 && Ho % 8 == 0 && Hi % 8 == 0 && Ho <= 1024 && Hi <= 1024;
}

}  // namespace wgf
}  // namespace hgnn

using namespace hgnn;

extern "C" int hgnn_wgrad_f32_workspace_bytes(int64_t M, int32_t Ho, int32_t Hi, size_t* bytes) {
    HGNN_REQUIRE(bytes != nullptr && M >= 0, "hgnn_wgrad_f32_workspace_bytes: bad argument");
    HGNN_REQUIRE(wgf::widths_ok(Ho, Hi),
                 "hgnn_wgrad_f32_workspace_bytes: Ho and Hi must be positive multiples of 8, at most 1024 (got %d, %d)",
                 Ho, Hi);
    const wgf::Shape s = wgf::shape_for(M, Ho, Hi);
    *bytes = (size_t)s.slices * (size_t)Ho * (size_t)Hi * sizeof(float);
    return HGNN_OK;
}

extern "C" int hgnn_wgrad_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t M, int32_t Ho,
                              int32_t Hi, float* out, int64_t ldo, void* workspace, size_t workspace_bytes,
                              hgnn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    HGNN_REQUIRE(M >= 0 && wgf::widths_ok(Ho, Hi),
                 "hgnn_wgrad_f32: Ho and Hi must be positive multiples of 8, at most 1024 (got %d, %d)", Ho, Hi);
    HGNN_REQUIRE(out != nullptr && ldo >= Hi, "hgnn_wgrad_f32: out is NULL or ldo < Hi");
    HGNN_REQUIRE(lda >= Ho && ldb >= Hi && lda % 4 == 0 && ldb % 4 == 0,
                 "hgnn_wgrad_f32: row strides must be multiples of 4 floats and cover the columns");
    HGNN_REQUIRE(M == 0 || (A != nullptr && B != nullptr && (uintptr_t)A % 16 == 0 && (uintptr_t)B % 16 == 0),
                 "hgnn_wgrad_f32: operands are NULL or not 16-byte aligned");
    const wgf::Shape s = wgf::shape_for(M, Ho, Hi);
    const size_t need = (size_t)s.slices * (size_t)Ho * (size_t)Hi * sizeof(float);
    HGNN_REQUIRE(workspace != nullptr && workspace_bytes >= need && (uintptr_t)workspace % 16 == 0,
                 "hgnn_wgrad_f32: workspace too small (%zu < %zu) or unaligned", workspace_bytes, need);
    if (M == 0) {   // an empty sum: zeros, nothing else
        HGNN_CHECK_HIP(hipMemset2DAsync(out, (size_t)ldo * sizeof(float), 0, (size_t)Hi * sizeof(float), (size_t)Ho, stream));
        return HGNN_OK;
    }
    float* partial = (float*)workspace;
    const dim3 grid((unsigned)s.tiles, (unsigned)s.slices);
#define HGNN_WGF(TO_, TI_, WO_, WI_)                                                                               \
    do {                                                                                                           \
        const size_t lds = 2 * wgf::KT * (size_t)((TO_ + 16) + (TI_ + 16)) * sizeof(float);                        \
        auto kern = wgf::k_wgrad_f32<TO_, TI_, WO_, WI_>;                                                          \
        HGNN_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
        kern<<<grid, WO_ * WI_ * 64, lds, stream>>>(A, lda, B, ldb, M, Ho, Hi, partial, s.rows_per_slice);         \
    } while (0)
    if (s.to == 256 && s.ti == 256) HGNN_WGF(256, 256, 2, 4);
    else if (s.to == 256) HGNN_WGF(256, 128, 4, 2);
    else HGNN_WGF(128, 128, 2, 2);
#undef HGNN_WGF
    wgf::k_wgrad_f32_reduce<<<(unsigned)ceil_div((int64_t)Ho * Hi, 256), 256, 0, stream>>>(partial, s.slices, Ho, Hi, out,
                                                                                          ldo);
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}
