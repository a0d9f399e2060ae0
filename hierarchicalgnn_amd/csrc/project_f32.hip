// The forward pre-projection of the EXACT fp32 route, hand-written for the fp32 MFMA:
//
//     out_b[r][h] = sum_k x[r][k] * w_b[h][k]        x: [M, K],  w_b: [N, K] (a Linear's weight, or a column block of it)
//
// for one or two weight blocks b from ONE launch (the source and the destination segment of an edge update read the
// same node table; hgnn_project_f32_split3 is the split-bf16 counterpart).  Every product is formed once by
// v_mfma_f32_16x16x4_f32, evaluated TRANSPOSED as in mlp_bwd_f32.hip's input form: D[h][r] = sum_k w[h][k] x[r][k], the
// row on the lane (lane & 15), the features in registers (h = 16 T + 4 (lane >> 4) + i), so a lane stores 16 bytes of
// its own output row per feature tile.  One wave owns 16 rows, four waves a 64-row tile.
//
// Order contract: every output element is the chain  acc = 0; acc = fmaf(x[r][k], w[h][k], acc)  for k ASCENDING.  The
// instruction chains its four k slots in order (slot = lane >> 4), so slot g of the q-th instruction of a 16-wide k
// chunk must hold k = k0 + 4 q + g.  That is why this file does not use mlp_f32_gemm.h's mma_chunk: its fragments hold
// four CONSECUTIVE k per lane (k = k0 + 4 g + q), which walks a chunk as 0, 4, 8, 12, 1, 5, ...  Here the weight chunk
// lies row-major in LDS ([feature][16 k], row stride 20 words) and is read one word at a time; the rows of x come from
// global memory as four single words per chunk (a 16-lane group reads 16 rows x 16 contiguous bytes).
//   * no split-K, no workspace, no atomics; the grid is (row tiles) x (blocks x feature passes), a pure function of
//     (M, N, number of blocks) -- never of the device;
//   * N up to 1024 in feature passes of at most 256 features (64 accumulator registers); the passes and the two blocks
//     are separate workgroups that re-read the same 64 rows of x, neighbours in launch order, from the cache;
//   * weight rows past N are staged as zeros and never stored; rows past M are clamped to the last row and never stored.
#include "mlp_common.h"

namespace hgnn {
namespace prj {

constexpr int NW = 4;
constexpr int WS = 20;   // LDS row stride of a weight chunk in words: 16 k + 4, rows stay 16-byte aligned

struct Args {
    const float* x;
    long long ldx, M;
    int K;
    const float* w[2];
    long long ldw;
    int N;
    float* out[2];
    long long ldo;
    int passes;   // feature passes per block
};

// NT feature tiles of 16 per pass
template <int NT>
__global__ __launch_bounds__(NW * 64) void k_project_f32(const Args a) {
    constexpr int FP = NT * 16;                     // features per pass
    constexpr int PIECES = FP * 4;                  // 16-byte pieces of one weight chunk
    constexpr int NP = (PIECES + NW * 64 - 1) / (NW * 64);
    __shared__ __attribute__((aligned(16))) float ws[2][FP * WS];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ei = lane & 15, g = lane >> 4;
    const int blk = (int)blockIdx.y / a.passes;
    const int h0 = ((int)blockIdx.y % a.passes) * FP;
    const float* __restrict__ W = a.w[blk];
    float* __restrict__ out = a.out[blk];
    const int nc = a.K / 16;

    const long long e = (long long)blockIdx.x * 64 + wave * 16 + ei;
    const bool valid = e < a.M;
    const float* px = a.x + (size_t)(valid ? e : a.M - 1) * (size_t)a.ldx + g;

    f32x4 rw[NP];
    auto load_w = [&](int c) {   // chunk c of the pass's weight rows; rows past N arrive as zeros
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int idx = tid + i * NW * 64;
            const int row = h0 + idx / 4;
            rw[i] = (idx < PIECES && row < a.N)
                        ? *(const f32x4*)(W + (size_t)row * (size_t)a.ldw + c * 16 + (idx & 3) * 4)
                        : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto store_w = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int idx = tid + i * NW * 64;
            if (idx < PIECES) *(f32x4*)(&ws[buf][(idx / 4) * WS + (idx & 3) * 4]) = rw[i];
        }
    };
    // slot g of instruction q holds k = 16 c + 4 q + g
    auto load_x = [&](int c, float (&v)[4]) {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = px[c * 16 + 4 * q];
    };

    f32x4 acc[NT];
#pragma unroll
    for (int T = 0; T < NT; ++T) acc[T] = f32x4{0.f, 0.f, 0.f, 0.f};

    float xc[4], xn[4];
    load_w(0);
    load_x(0, xc);
    store_w(0);
    __syncthreads();
    for (int c = 0; c < nc; ++c) {   // nc is uniform over the workgroup: every wave takes every barrier
        const bool more = c + 1 < nc;
        if (more) {
            load_w(c + 1);
            load_x(c + 1, xn);
        }
        const float* wt = &ws[c & 1][ei * WS + g];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            // consecutive MFMAs write different accumulators (dependent latency 40 cycles against a 32-cycle issue)
#pragma unroll
            for (int T = 0; T < NT; ++T)
                acc[T] = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[T * 16 * WS + 4 * q], xc[q], acc[T], 0, 0, 0);
        }
        if (more) {
            store_w((c + 1) & 1);
#pragma unroll
            for (int q = 0; q < 4; ++q) xc[q] = xn[q];
        }
        __syncthreads();
    }
    // D layout: column (row of x) = lane & 15, rows (features) = 4 * (lane >> 4) + i
    if (valid) {
        float* op = out + (size_t)e * (size_t)a.ldo + h0 + g * 4;
#pragma unroll
        for (int T = 0; T < NT; ++T)
            if (h0 + T * 16 < a.N) *(f32x4*)(op + T * 16) = acc[T];
    }
}

// features per pass: a pure function of N (tests/exact_tail_ref.py restates it)
static int pass_width(int N) { return N <= 16 ? 16 : N <= 32 ? 32 : N <= 64 ? 64 : N <= 128 ? 128 : 256; }

template <int NT>
static int launch(const Args& a, int blocks, hipStream_t s) {
    const dim3 grid((unsigned)ceil_div(a.M, 64), (unsigned)(blocks * a.passes));
    k_project_f32<NT><<<grid, NW * 64, 0, s>>>(a);
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}

}  // namespace prj
}  // namespace hgnn

using namespace hgnn;

extern "C" int hgnn_project_f32(const float* x, int64_t ldx, int64_t M, int32_t K, const float* w0, const float* w1,
                                int64_t ldw, int32_t N, float* out0, float* out1, int64_t ldo, hgnn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    static const char fn[] = "hgnn_project_f32";
    if (K < 16 || K > 512 || K % 16 != 0 || N < 16 || N > 1024 || N % 16 != 0) {
        set_error("%s: unsupported shape K=%d N=%d (K a multiple of 16 in [16, 512], N a multiple of 16 in [16, 1024])", fn,
                  K, N);
        return HGNN_ERR_UNSUPPORTED;
    }
    HGNN_REQUIRE(M >= 0 && M <= 0x7fffffffLL, "%s: bad M", fn);
    HGNN_REQUIRE((w1 == nullptr) == (out1 == nullptr), "%s: w1 and out1 are given together or not at all", fn);
    HGNN_REQUIRE(ldx >= K && ldw >= K && ldo >= N && ldx % 4 == 0 && ldw % 4 == 0 && ldo % 4 == 0,
                 "%s: row strides must be multiples of 4 floats and cover the columns", fn);
    HGNN_REQUIRE(w0 != nullptr && out0 != nullptr && (M == 0 || x != nullptr), "%s: NULL pointer", fn);
    HGNN_REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)w0 % 16 == 0 && (uintptr_t)w1 % 16 == 0 &&
                     (uintptr_t)out0 % 16 == 0 && (uintptr_t)out1 % 16 == 0,
                 "%s: pointers must be 16-byte aligned", fn);
    if (M == 0) return HGNN_OK;
    prj::Args a;
    a.x = x;
    a.ldx = ldx;
    a.M = M;
    a.K = K;
    a.w[0] = w0;
    a.w[1] = w1;
    a.ldw = ldw;
    a.N = N;
    a.out[0] = out0;
    a.out[1] = out1;
    a.ldo = ldo;
    const int fp = prj::pass_width(N);
    a.passes = (N + fp - 1) / fp;
    const int blocks = w1 != nullptr ? 2 : 1;
    switch (fp) {
        case 16: return prj::launch<1>(a, blocks, stream);
        case 32: return prj::launch<2>(a, blocks, stream);
        case 64: return prj::launch<4>(a, blocks, stream);
        case 128: return prj::launch<8>(a, blocks, stream);
        default: return prj::launch<16>(a, blocks, stream);
    }
}
