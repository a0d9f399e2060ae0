// Fused backward of ONE layer boundary of the EXACT fp32 training path (hand-written data gradient on fp32 MFMA):
//
//   LayerNorm form:  da   = dz . W                       [M, K] x [K, N]   (W = the Linear's weight [K out, N in])
//                    dz'  = dLayerNorm(act'(LN(z')) * da)                   z' = the previous layer's pre-LayerNorm rows
//                    a'   = act(LN(z'))                                    (what the weight gradient of W needs)
//                    + per-workgroup column partials of dgamma' / dbeta' / dbias' (column sums of dz')
//   input form    :  dx   = dz . W (+ skip)                                first layer: gradient of a direct input segment,
//                                                                          the skip connection's gradient added in place
//
// i.e. the data-gradient GEMM of Modules/utils.py:169-196's Linear fused with the LayerNorm / activation backward of
// the layer below it.  Unfused this is one library GEMM writing da, hgnn_ln_act_backward_f32 reading z' and da and
// writing dz', and hgnn_ln_act_forward_f32 reading z' once more for a'.
//
// The GEMM is the fused forward's (mlp_fused.hip) single layer with W^T as the weight, the rows of dz as the input and
// no bias: v_mfma_f32_16x16x4_f32 evaluated TRANSPOSED, D[n][e] = sum_k W^T[n][k] dz[e][k], so the row sits on the lane
// (col = lane & 15) and the features in registers (n = 16 T + 4 (lane >> 4) + r).  One wave owns 16 rows and ALL N
// features, four waves make a 64-row tile; W^T streams through LDS in k-chunks of 16 (LDS-DMA, double buffered, one
// barrier per chunk), the rows of dz come straight from global memory in the B-operand layout.  The epilogue works in
// the accumulator layout:
//   * LayerNorm statistics of z' (centred: mean first, then sum((z' - mean)^2)) and the two row sums of the LayerNorm
//     backward are in-register sums plus two cross-lane adds -- nothing crosses waves;
//   * dgamma' / dbeta' / dbias' : the 16 values a lane holds of four feature tiles are reduced over the 16 row lanes
//     by a halving exchange (8 + 4 + 2 + 1 shuffles for 16 columns) that leaves column v of the group on lane v --
//     the one lane that owns the column -- which carries the sum in a register across all tiles of the workgroup.
//     At the end the four waves' sums are added in wave order through LDS and written once.  No atomics.
//   * workgroups are persistent over the 64-row tiles in a fixed order on a constant grid (HGNN_MLP_BWD_F32_BLOCKS):
//     the same inputs give the same bits on any device.
//   * z' (as xhat after the statistics) stays in registers between the epilogue phases.  N = 512 (128 accumulators +
//     128 registers of z') runs one workgroup per CU on the unified 512-register file, the narrower widths two.
//     Tried and not shipped: N = 512 re-reading z' in every phase at two workgroups per CU (spills 22-27 registers).
#include "mlp_common.h"
#include "mlp_f32_gemm.h"

namespace hgnn {
namespace bwf {

constexpr int NW = 4;
constexpr int kGrid = HGNN_MLP_BWD_F32_BLOCKS;

struct Args {
    const float* dz;      // [M, K]
    int K;
    const float* Wt;      // W^T [N][K] row-major
    const float* z_prev;  // [M, N] (LayerNorm form)
    const float* lnw;
    const float* lnb;
    int act;
    float eps;
    const float* skip;    // [M, N] or NULL (input form)
    float* out;           // [M, N]: dz' (LayerNorm form) / dx (input form)
    float* a_prev;        // [M, N] or NULL (LayerNorm form)
    float* partials;      // [kGrid][3][N] (LayerNorm form)
    long long M;
};

__device__ __forceinline__ f32x4 shfl4_xor(f32x4 v, int m) {
    f32x4 o;
    o.x = __shfl_xor(v.x, m);
    o.y = __shfl_xor(v.y, m);
    o.z = __shfl_xor(v.z, m);
    o.w = __shfl_xor(v.w, m);
    return o;
}

// t0 .. t3 hold, per lane, this lane's row of the 16 columns v = 4 tt + r of a column group (four feature tiles); the
// result is the sum over the 16 row lanes (lane & 15) of column v = lane & 15: each exchange hands half of the columns
// to the partner lane, 8 + 4 + 2 + 1 shuffles.  Selects are on VALUES (named registers), never on an index.
__device__ __forceinline__ float lanes16_scatter_sum(f32x4 t0, f32x4 t1, f32x4 t2, f32x4 t3, int ei) {
    const bool u8 = (ei & 8) != 0, u4 = (ei & 4) != 0, u2 = (ei & 2) != 0, u1 = (ei & 1) != 0;
    const f32x4 p = (u8 ? t2 : t0) + shfl4_xor(u8 ? t0 : t2, 8);   // columns 0-3 (8-11 on the upper lanes)
    const f32x4 q = (u8 ? t3 : t1) + shfl4_xor(u8 ? t1 : t3, 8);   // columns 4-7 (12-15)
    const f32x4 w = (u4 ? q : p) + shfl4_xor(u4 ? p : q, 4);
    const float a = (u2 ? w.z : w.x) + __shfl_xor(u2 ? w.x : w.z, 2);
    const float b = (u2 ? w.w : w.y) + __shfl_xor(u2 ? w.y : w.w, 2);
    return (u1 ? b : a) + __shfl_xor(u1 ? a : b, 1);
}

template <int NG>
__device__ __forceinline__ float tree_sum(float (&p)[NG]) {
#pragma unroll
    for (int w = NG / 2; w >= 1; w >>= 1)
#pragma unroll
        for (int i = 0; i < w; ++i) p[i] += p[i + w];
    return p[0];
}

// ACT: compile-time activation code of the LayerNorm form (-1: read it from the arguments)
template <int NT, int MINW, bool LNF, int ACT>
__global__ __launch_bounds__(NW * 64, MINW) void k_mlp_bwd_f32(const Args a) {
    static_assert(NT % 4 == 0, "column sums are exchanged in groups of four feature tiles");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int N = NT * 16;
    constexpr int BUF = NT * 256;  // floats per chunk buffer
    constexpr int NG = NT / 4;     // column groups of 64 features: lane (ei, g) owns column 64 G + 16 (ei >> 2) + 4 g + (ei & 3)
    constexpr float inv_n = 1.0f / (float)N;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ei = lane & 15;
    const int g = lane >> 4;
    const int nc = a.K / 16;
    const int n_pieces = pieces_of<N, NW>(wave);
    const long long n_tiles = (a.M + 63) / 64;
    const int code = ACT >= 0 ? ACT : a.act;

    float cs_dg[LNF ? NG : 1], cs_db[LNF ? NG : 1], cs_dz[LNF ? NG : 1];
#pragma unroll
    for (int G = 0; G < (LNF ? NG : 1); ++G) cs_dg[G] = cs_db[G] = cs_dz[G] = 0.f;

    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {   // uniform trip count per workgroup
        // The tile loop keeps NOTHING derived from the argument pointers live across its iterations: hipcc would otherwise
        // hoist every per-lane address of a tile (eight weight-piece sources, the parameter and row pointers) out of
        // the loop, ~40 registers held through the MFMA loop and the epilogue.  A zero the compiler cannot see through,
        // renewed once per tile, is added to each base pointer; the addresses are a few VALU instructions per 64 rows.
        size_t opaque0 = 0;
        asm volatile("" : "+s"(opaque0));
        const float* p_dz = a.dz + opaque0;
        const float* p_wt = a.Wt + opaque0;
        const float* p_z = a.z_prev + opaque0;
        const float* p_lnw = a.lnw + opaque0;
        const float* p_lnb = a.lnb + opaque0;
        const float* p_skip = a.skip + opaque0;
        float* p_out = a.out + opaque0;
        float* p_a = a.a_prev + opaque0;
        const long long e = tile * 64 + wave * 16 + ei;
        const bool valid = e < a.M;
        const long long er = valid ? e : a.M - 1;
        const size_t off = (size_t)er * N + g * 4;

        // ---------------- da = dz . W : weights through LDS, the rows of dz from global memory
        f32x4 acc[NT];
#pragma unroll
        for (int T = 0; T < NT; ++T) acc[T] = f32x4{0.f, 0.f, 0.f, 0.f};
        __builtin_amdgcn_s_setprio(2);
        {
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            const float* px = p_dz + (size_t)er * (size_t)a.K + g * 4;
            __syncthreads();  // everyone is done with both buffers of the previous tile
            stage_w<N, NW>(p_wt, a.K, 0, lds, wave, lane);
            f32x4 x0 = *(const f32x4*)px;
            f32x4 x1 = nc > 1 ? *(const f32x4*)(px + 16) : zero;
            px += 32;
            for (int c = 0; c < nc; ++c) {
                wait_dma();        // this wave's pieces of chunk c have landed
                __syncthreads();   // everyone's have; buffer (c+1)&1 is free again
                const f32x4 x2 = c + 2 < nc ? *(const f32x4*)px : zero;
                px += 16;
                const float* wb = lds + (c & 1) * BUF + lane * 4;
                WStage st = begin_stage<NW>(p_wt, a.K, (c + 1) * 16, lds + ((c + 1) & 1) * BUF, wave, lane);
                mma_chunk<NT, N, NW>(acc, wb, x0, st, c + 1 < nc ? n_pieces : 0);
                x0 = x1;
                x1 = x2;
            }
        }
        __builtin_amdgcn_s_setprio(0);

        if constexpr (!LNF) {
            if (valid) {
                float* op = p_out + off;
                if (a.skip != nullptr) {
                    const float* sp = p_skip + off;
#pragma unroll
                    for (int T = 0; T < NT; ++T) *(f32x4*)(op + T * 16) = acc[T] + *(const f32x4*)(sp + T * 16);
                } else {
#pragma unroll
                    for (int T = 0; T < NT; ++T) *(f32x4*)(op + T * 16) = acc[T];
                }
            }
        } else {
            // ---- E1: the previous layer's pre-LayerNorm rows in the accumulator layout, centred row statistics
            const float* zp = p_z + off;
            f32x4 zr[NT];   // z', then z' - mean, then xhat
            // row sums: a lane adds the 16 values of a column group in sequence, the groups' sums are combined by a halving
            // tree (one chain over all N / 4 values of a lane rounds at the magnitude of an offset row N / 64 times as often)
            float part[NG];
#pragma unroll
            for (int G = 0; G < NG; ++G) {
                float t = 0.f;
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    const f32x4 x = *(const f32x4*)(zp + (G * 4 + tt) * 16);
                    zr[G * 4 + tt] = x;
                    t += (x.x + x.y) + (x.z + x.w);
                }
                part[G] = t;
            }
            float s = tree_sum<NG>(part);
            s += __shfl_xor(s, 16);
            s += __shfl_xor(s, 32);
            const float mean = s * inv_n;
#pragma unroll
            for (int G = 0; G < NG; ++G) {
                float t = 0.f;
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    const f32x4 d = zr[G * 4 + tt] - mean;
                    zr[G * 4 + tt] = d;
                    t += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
                }
                part[G] = t;
            }
            float q = tree_sum<NG>(part);
            q += __shfl_xor(q, 16);
            q += __shfl_xor(q, 32);
            const float rstd = 1.0f / sqrtf(q * inv_n + a.eps);
            // ---- E2: activation', gamma; column sums of dgamma / dbeta; row sums of the LayerNorm backward
            float sg = 0.f, sgx = 0.f;
#pragma unroll
            for (int G = 0; G < NG; ++G) {
                f32x4 vg[4], vb[4];
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    const int T = G * 4 + tt;
                    const f32x4 lw = *(const f32x4*)(p_lnw + T * 16 + g * 4);
                    const f32x4 lb = *(const f32x4*)(p_lnb + T * 16 + g * 4);
                    const f32x4 xh = zr[T] * rstd;
                    zr[T] = xh;
                    f32x4 av, gg;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float y = fmaf(xh[r], lw[r], lb[r]);
                        float ac, gr;
                        act_val_grad(y, code, ac, gr);
                        const float dy = valid ? acc[T][r] * gr : 0.f;
                        av[r] = ac;
                        vg[tt][r] = dy * xh[r];
                        vb[tt][r] = dy;
                        const float gv = dy * lw[r];
                        gg[r] = gv;
                        sg += gv;
                        sgx = fmaf(gv, xh[r], sgx);
                        // two activations at a time: all 16 of a tile interleaved hold ~8 temporaries each
                        if (r == 1) __builtin_amdgcn_sched_barrier(0);
                    }
                    acc[T] = gg;
                    if (a.a_prev != nullptr && valid) *(f32x4*)(p_a + off + T * 16) = av;
                    // the two row sums are serial chains used only after the phase: left alone, hipcc sinks the whole
                    // chain to the end of the phase and keeps every tile's xhat alive for it
                    asm volatile("" : "+v"(sg), "+v"(sgx));
                    // one feature tile at a time: interleaving the four tiles of a group keeps ~30 registers live
                    // per tile on top of the accumulators and z'
                    __builtin_amdgcn_sched_barrier(0);
                }
                cs_dg[G] += lanes16_scatter_sum(vg[0], vg[1], vg[2], vg[3], ei);
                cs_db[G] += lanes16_scatter_sum(vb[0], vb[1], vb[2], vb[3], ei);
                // one column group at a time: keeps hipcc from hoisting every group's parameter loads to the top of
                // the phase
                asm volatile("" ::: "memory");
            }
            sg += __shfl_xor(sg, 16);
            sgx += __shfl_xor(sgx, 16);
            sg += __shfl_xor(sg, 32);
            sgx += __shfl_xor(sgx, 32);
            const float mg = sg * inv_n, mgx = sgx * inv_n;
            // ---- E3: dz' = rstd * (g - mean(g) - xhat * mean(g * xhat)); column sums of dz' (the bias gradient)
#pragma unroll
            for (int G = 0; G < NG; ++G) {
                f32x4 vz[4];
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    const int T = G * 4 + tt;
                    const f32x4 xh = zr[T];
                    f32x4 o;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        o[r] = rstd * (acc[T][r] - mg - xh[r] * mgx);
                        vz[tt][r] = valid ? o[r] : 0.f;
                    }
                    if (valid) *(f32x4*)(p_out + off + T * 16) = o;
                    __builtin_amdgcn_sched_barrier(0);
                }
                cs_dz[G] += lanes16_scatter_sum(vz[0], vz[1], vz[2], vz[3], ei);
                asm volatile("" ::: "memory");
            }
        }
    }

    if constexpr (LNF) {
        // the four waves' column sums, added in wave order: red[wave][3][N] reuses the weight buffers
        __syncthreads();
#pragma unroll
        for (int G = 0; G < NG; ++G) {
            const int col = G * 64 + (ei >> 2) * 16 + g * 4 + (ei & 3);
            float* r = lds + wave * 3 * N + col;
            r[0] = cs_dg[G];
            r[N] = cs_db[G];
            r[2 * N] = cs_dz[G];
        }
        __syncthreads();
        for (int i = threadIdx.x; i < 3 * N; i += NW * 64)
            a.partials[(size_t)blockIdx.x * 3 * N + i] = ((lds[i] + lds[3 * N + i]) + lds[6 * N + i]) + lds[9 * N + i];
    }
}

template <int NT, int MINW, bool LNF, int ACT>
static int launch_act(const Args& a, hipStream_t s) {
    const size_t lds_bytes = (size_t)2 * NT * 256 * sizeof(float);   // >= the 4 x 3 x N floats of the final exchange
    const long long n_tiles = (a.M + 63) / 64;
    // LayerNorm form: a fixed grid (the partials are [HGNN_MLP_BWD_F32_BLOCKS][3][N]; idle workgroups write zeros)
    const unsigned grid = LNF ? (unsigned)kGrid : (unsigned)(n_tiles < kGrid ? n_tiles : kGrid);
    static_assert((size_t)2 * NT * 256 * sizeof(float) <= 64 * 1024, "above 64 KiB the launch needs hipFuncSetAttribute");
    k_mlp_bwd_f32<NT, MINW, LNF, ACT><<<grid, NW * 64, lds_bytes, s>>>(a);
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}

template <int NT, int MINW>
static int launch(const Args& a, hipStream_t s) {
    if (a.z_prev == nullptr) return launch_act<NT, MINW, false, HGNN_ACT_NONE>(a, s);
    switch (a.act) {   // the hidden layers of every network are GELU; Tanh closes the two-layer ones
        case HGNN_ACT_GELU: return launch_act<NT, MINW, true, HGNN_ACT_GELU>(a, s);
        case HGNN_ACT_TANH: return launch_act<NT, MINW, true, HGNN_ACT_TANH>(a, s);
        case HGNN_ACT_SILU: return launch_act<NT, MINW, true, HGNN_ACT_SILU>(a, s);   // hidden_activation: SiLU
    }
    return launch_act<NT, MINW, true, -1>(a, s);
}

}  // namespace bwf
}  // namespace hgnn

using namespace hgnn;

extern "C" int hgnn_mlp_backward_layer_supported_f32(int32_t K, int32_t N) {
    return (K >= 64 && K <= 1024 && K % 16 == 0 && (N == 64 || N == 128 || N == 256 || N == 512)) ? 1 : 0;
}

extern "C" int hgnn_mlp_backward_layer_f32(const float* dz, int64_t M, int32_t K, int32_t N, const float* Wt,
                                           const float* z_prev, const float* ln_w, const float* ln_b, int32_t act,
                                           float eps, const float* skip, float* out, float* a_prev, float* partials,
                                           hgnn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    static const char fn[] = "hgnn_mlp_backward_layer_f32";
    if (!hgnn_mlp_backward_layer_supported_f32(K, N)) {
        set_error("%s: unsupported shape K=%d N=%d (K a multiple of 16 in [64, 1024], N in {64, 128, 256, 512})", fn, K, N);
        return HGNN_ERR_UNSUPPORTED;
    }
    HGNN_REQUIRE(M >= 0 && M <= 0x7fffffffLL, "%s: bad M", fn);
    const bool ln = z_prev != nullptr;
    HGNN_REQUIRE(!ln || (ln_w != nullptr && ln_b != nullptr && partials != nullptr && skip == nullptr),
                 "%s: the LayerNorm form needs ln_w, ln_b, partials and no skip", fn);
    HGNN_REQUIRE(ln || (a_prev == nullptr && partials == nullptr), "%s: a_prev / partials belong to the LayerNorm form", fn);
    HGNN_REQUIRE(act >= HGNN_ACT_NONE && act <= HGNN_ACT_LAST, "%s: unknown activation code %d", fn, act);
    if (M == 0 && !ln) return HGNN_OK;
    HGNN_REQUIRE(M == 0 || (dz != nullptr && Wt != nullptr && out != nullptr), "%s: NULL pointer", fn);
    HGNN_REQUIRE((uintptr_t)dz % 16 == 0 && (uintptr_t)Wt % 16 == 0 && (uintptr_t)z_prev % 16 == 0 &&
                     (uintptr_t)skip % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)a_prev % 16 == 0 &&
                     (uintptr_t)ln_w % 16 == 0 && (uintptr_t)ln_b % 16 == 0 && (uintptr_t)partials % 16 == 0,
                 "%s: pointers must be 16-byte aligned", fn);
    bwf::Args a;
    a.dz = dz;
    a.K = K;
    a.Wt = Wt;
    a.z_prev = z_prev;
    a.lnw = ln_w;
    a.lnb = ln_b;
    a.act = act;
    a.eps = eps;
    a.skip = skip;
    a.out = out;
    a.a_prev = a_prev;
    a.partials = partials;
    a.M = M;
    // M == 0 in the LayerNorm form still runs: every workgroup writes its (zero) partials
    switch (N) {
        case 64: return bwf::launch<4, 2>(a, stream);
        case 128: return bwf::launch<8, 2>(a, stream);
        case 256: return bwf::launch<16, 2>(a, stream);
        case 512: return bwf::launch<32, 1>(a, stream);
    }
    set_error("%s: no instantiation", fn);
    return HGNN_ERR_UNSUPPORTED;
}
