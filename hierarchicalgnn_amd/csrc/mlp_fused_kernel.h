// The fused fp32 MLP kernel template (k_fused_mlp), its argument struct and launch helpers, shared by the
// translation units that instantiate it: mlp_fused.hip (the native grid K -> 2L (-> 2L) -> L, heads, PLAIN and PAD
// kernels) and mlp_fused_square.hip (hidden = output).  The mapping is described at the top of mlp_fused.hip.
// Everything here is a template or static: each translation unit compiles only the instantiations it launches.
#pragma once
#include "mlp_common.h"
#include "mlp_f32_gemm.h"
#include "mlp_desc.h"
#include "options.h"

namespace hgnn {

struct MlpArgs {
    const float* seg_table[3];
    const int32_t* seg_index[3];
    int seg_width[3];
    int n_seg;
    int K1;       // columns stored in W[0] (multiple of 16)
    int K1_real;  // concatenated input width; < K1 only in small-K mode (K1_real <= 16, W[0] zero padded)
    int n_out_real;  // real output columns; < (tiles of the last layer)*16 only for PARTIAL kernels (heads with a
                     // plain 1- or emb_dim-wide last layer, supernode encoder L-8): W/b/ln of the last layer are
                     // zero padded to the tile width, statistics and stores use the real width
    const float* W[3];
    const float* b[3];
    const float* lnw[3];
    const float* lnb[3];
    int act[3];
    float eps;
    const float* skip;
    float* out;
    float* save_pre[3];  // optional [M, width_l] dumps of each layer's pre-LayerNorm output (training)
    const float* pre_table[2];    // pre-projected gathered segments [rows, NT1*16] (see hgnn_mlp_desc.n_pre)
    const int32_t* pre_index[2];
    int n_pre;
    long long M;
    int ablate;        // DIAGNOSTIC ONLY (wrong results): 1 = skip LN/act, 2 = skip weight DMA, 4 = skip barriers
    int real[3];       // PAD kernels only: real output width of every layer (<= its tile width; the rest is zero padding)
};

// acc[T][r] (edge = lane&15, feature = 16T + 4*(lane>>4) + r): LayerNorm over features, then act
// PARTIAL: only n_real < NT*16 features are real; the padded ones have zero weights and bias, so their
// accumulators are exactly 0: they add nothing to the sum and mean^2 each to the squared deviations
// MASK (the PAD kernels, any number of padded tiles): the padded features are left out of the centred pass instead
// (n_real % 4 == 0: a lane's four features of a tile are all real or all padding), nothing is corrected afterwards --
// at up to 7 padded tiles  pad * mean^2  cancels badly against q on a row with an offset.  Their ln_w / ln_b are
// zero, so they come out as exactly 0 and feed zeros into the next layer.
template <int NT, int ACT, bool LN = true, bool PARTIAL = false, bool MASK = false>
__device__ __forceinline__ void layernorm_act(f32x4 (&acc)[NT], const float* __restrict__ lnw,
                                              const float* __restrict__ lnb, int act, float eps, int g,
                                              int n_real = NT * 16) {
    static_assert(!(PARTIAL && MASK), "one treatment of the padded features");
    if (!LN) return;  // plain last layer of a head: bias only
    const float inv_n = (PARTIAL || MASK) ? 1.0f / (float)n_real : 1.0f / (float)(NT * 16);
    float s = 0.f;
#pragma unroll
    for (int T = 0; T < NT; ++T) s += (acc[T].x + acc[T].y) + (acc[T].z + acc[T].w);
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    // MASK: n_real is no power of two, 1 / n_real is rounded: a true division keeps the mean of a constant row exact
    // (its deviations exactly 0), as s * 2^-k does on the grid widths
    const float mean = MASK ? s / (float)n_real : s * inv_n;
    float q = 0.f;
#pragma unroll
    for (int T = 0; T < NT; ++T) {
        f32x4 d = acc[T] - mean;
        if constexpr (MASK) {
            const float t = (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
            q += (T * 16 + g * 4 < n_real) ? t : 0.f;
        } else {
            q += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
        }
    }
    q += __shfl_xor(q, 16);
    q += __shfl_xor(q, 32);
    if (PARTIAL) q -= (float)(NT * 16 - n_real) * mean * mean;
    const float rstd = 1.0f / sqrtf((MASK ? q / (float)n_real : q * inv_n) + eps);
#pragma unroll
    for (int T = 0; T < NT; ++T) {
        const f32x4 w4 = *(const f32x4*)(lnw + T * 16 + g * 4);
        const f32x4 b4 = *(const f32x4*)(lnb + T * 16 + g * 4);
        f32x4 v = (acc[T] - mean) * rstd * w4 + b4;
        const int code = ACT >= 0 ? ACT : act;  // compile-time for the common networks
        v.x = act_apply(v.x, code);
        v.y = act_apply(v.y, code);
        v.z = act_apply(v.z, code);
        v.w = act_apply(v.w, code);
        acc[T] = v;
    }
}

// a LayerNorm-less layer (PLAIN kernels, hgnn_mlp_forward_f32_plain): act on the bias-initialised accumulators, no
// statistics.  Zero-padded features of a narrow last layer come out as act(0); its store masks them
template <int NT>
__device__ __forceinline__ void act_only(f32x4 (&acc)[NT], int act) {
#pragma unroll
    for (int T = 0; T < NT; ++T) {
        acc[T].x = act_apply(acc[T].x, act);
        acc[T].y = act_apply(acc[T].y, act);
        acc[T].z = act_apply(acc[T].z, act);
        acc[T].w = act_apply(acc[T].w, act);
    }
}

template <int NT>
__device__ __forceinline__ void init_bias(f32x4 (&acc)[NT], const float* __restrict__ b, int g) {
#pragma unroll
    for (int T = 0; T < NT; ++T) acc[T] = *(const f32x4*)(b + T * 16 + g * 4);
}

// one register-resident layer: out[NTO tiles] = W[NTO*16][NTI*16] * in  (in = previous accumulators)
template <int NTI, int NTO, int NW>
__device__ __forceinline__ void dense_from_regs(const f32x4 (&in)[NTI], f32x4 (&out)[NTO],
                                                const float* __restrict__ W, float* lds, int wave, int lane,
                                                int ablate) {
    constexpr int KD = NTI * 16;
    constexpr int BUF = NTO * 256;  // floats per chunk buffer
    const int n_pieces = pieces_of<NTO * 16, NW>(wave);
    __syncthreads();                // everyone is done with both buffers of the previous layer
    stage_w<NTO * 16, NW>(W, KD, 0, lds, wave, lane);
#pragma unroll
    for (int c = 0; c < NTI; ++c) {
        wait_dma();                           // this wave's pieces of chunk c have landed
        if (!(ablate & 4)) __syncthreads();   // everyone's have; buffer (c+1)&1 is free again
        const float* wb = lds + (c & 1) * BUF + lane * 4;
        WStage st = begin_stage<NW>(W, KD, (c + 1) * 16, lds + ((c + 1) & 1) * BUF, wave, lane);
        mma_chunk<NTO, NTO * 16, NW>(out, wb, in[c], st, (c + 1 < NTI && !(ablate & 2)) ? n_pieces : 0);
    }
}

template <int NT, bool PARTIAL = false>
__device__ __forceinline__ void store_out(const f32x4 (&acc)[NT], const MlpArgs& a, long long e, bool valid,
                                          int g) {
    if (!valid) return;
    if constexpr (PARTIAL) {  // out[e][0 .. n_out_real): the columns past the real width are padding
        const int nr = a.n_out_real;
        float* op = a.out + (size_t)e * (size_t)nr;
        if ((nr & 3) == 0) {
#pragma unroll
            for (int T = 0; T < NT; ++T) {
                const int col = T * 16 + g * 4;
                if (col < nr) *(f32x4*)(op + col) = acc[T];
            }
        } else {
#pragma unroll
            for (int T = 0; T < NT; ++T) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int col = T * 16 + g * 4 + r;
                    if (col < nr) op[col] = acc[T][r];
                }
            }
        }
        return;
    }
    constexpr int NOUT = NT * 16;
    float* op = a.out + (size_t)e * NOUT + g * 4;
    if (a.skip != nullptr) {
        const float* sp = a.skip + (size_t)e * NOUT + g * 4;
#pragma unroll
        for (int T = 0; T < NT; ++T) *(f32x4*)(op + T * 16) = acc[T] + *(const f32x4*)(sp + T * 16);
    } else {
#pragma unroll
        for (int T = 0; T < NT; ++T) *(f32x4*)(op + T * 16) = acc[T];
    }
}

// PAD kernels: out[e][0 .. n_out_real) (+ skip rows of the same width), 16-byte pieces (n_out_real % 4 == 0)
template <int NT>
__device__ __forceinline__ void store_out_pad(const f32x4 (&acc)[NT], const MlpArgs& a, long long e, bool valid,
                                              int g) {
    if (!valid) return;
    const int nr = a.n_out_real;
    float* op = a.out + (size_t)e * (size_t)nr;
    if (a.skip != nullptr) {
        const float* sp = a.skip + (size_t)e * (size_t)nr;
#pragma unroll
        for (int T = 0; T < NT; ++T) {
            const int col = T * 16 + g * 4;
            if (col < nr) *(f32x4*)(op + col) = acc[T] + *(const f32x4*)(sp + col);
        }
    } else {
#pragma unroll
        for (int T = 0; T < NT; ++T) {
            const int col = T * 16 + g * 4;
            if (col < nr) *(f32x4*)(op + col) = acc[T];
        }
    }
}

// training: dump a layer's pre-LayerNorm activations z[e][f] (what the hand-written backward in
// fused.py needs; the hidden activations themselves are recomputed from it, never stored)
// PAD: rows of `real` floats (real % 4 == 0), the padded features are not written
template <int NT, bool PAD = false>
__device__ __forceinline__ void dump_pre(const f32x4 (&acc)[NT], float* base, long long e, bool valid, int g,
                                         int real = NT * 16) {
    if (base == nullptr || !valid) return;  // base is wave-uniform
    if constexpr (PAD) {
        float* rp = base + (size_t)e * (size_t)real;
#pragma unroll
        for (int T = 0; T < NT; ++T) {
            const int col = T * 16 + g * 4;
            if (col < real) *(f32x4*)(rp + col) = acc[T];
        }
        return;
    }
    float* op = base + (size_t)e * (NT * 16) + g * 4;
#pragma unroll
    for (int T = 0; T < NT; ++T) *(f32x4*)(op + T * 16) = acc[T];
}

// NT1/NT2/NT3: 16-feature tiles of layer 1 / 2 / 3 outputs (NT3 == 0: two-layer MLP)
// ACT_H / ACT_O: activation of the hidden layers / of the last layer (HGNN_ACT_*), or -1 = read
// it from the descriptor per element (keeps rare combinations working without an instantiation)
// PLAIN_LAST: the last layer has no LayerNorm / activation (classifier heads, width-1 output)
// PARTIAL: the last layer's real width is a.n_out_real < its tile width (see MlpArgs)
// PAD: EVERY layer's real width a.real[l] may be below its tile width (widths between the template grid's: weights,
// biases and LayerNorm parameters zero padded, W[l >= 1] also in its columns); statistics are masked, dumps, skip
// and stores use the real row strides.  False for every kernel of the native grid: their code does not depend on it.
// PLAIN: no layer has a LayerNorm (make_mlp with layer_norm=False): each layer is act(x W^T + b), the activation code
// read from the descriptor; PARTIAL is then only the store mask of a narrow last layer.  False everywhere else.
template <int NT1, int NT2, int NT3, int MINW, int ACT_H, int ACT_O, bool PLAIN_LAST = false, int NW = 4,
          bool PARTIAL = false, bool PAD = false, bool PLAIN = false>
__global__ __launch_bounds__(NW * 64, MINW) void k_fused_mlp(const MlpArgs a) {
    static_assert(!PAD || (PARTIAL == PLAIN_LAST && (NT2 > 0 || !PARTIAL)), "PAD: heads keep the PARTIAL store");
    static_assert(!PLAIN || (NT2 > 0 && !PAD && ACT_H < 0), "PLAIN: 2 or 3 layers of the native grid, runtime codes");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ei = lane & 15;
    const int g = lane >> 4;
    const long long e = (long long)blockIdx.x * (NW * 16) + wave * 16 + ei;
    const bool valid = e < a.M;
    const long long er = valid ? e : 0;

    // per-lane row start of every input segment (the gather is folded in here).  The X stream is
    // read through ONE running pointer that hops to the next segment's row at a segment boundary,
    // so nothing is runtime-indexed (cdna_hip_programming.md 5.4 rule 20).
    const float* q0;
    const float* q1;
    const float* q2;
    {
        long long r = a.seg_index[0] != nullptr ? (long long)a.seg_index[0][er] : er;
        q0 = a.seg_table[0] + (size_t)(r < 0 ? 0 : r) * (size_t)a.seg_width[0] + g * 4;
        q1 = q0;
        q2 = q0;
        if (a.n_seg > 1) {
            r = a.seg_index[1] != nullptr ? (long long)a.seg_index[1][er] : er;
            q1 = a.seg_table[1] + (size_t)(r < 0 ? 0 : r) * (size_t)a.seg_width[1] + g * 4;
        }
        if (a.n_seg > 2) {
            r = a.seg_index[2] != nullptr ? (long long)a.seg_index[2][er] : er;
            q2 = a.seg_table[2] + (size_t)(r < 0 ? 0 : r) * (size_t)a.seg_width[2] + g * 4;
        }
    }
    const int nc = a.K1 / 16;
    const int c1 = a.seg_width[0] / 16;                       // first chunk of segment 1
    const int c2 = c1 + (a.n_seg > 1 ? a.seg_width[1] / 16 : nc);  // first chunk of segment 2
    const float* px = q0;
    int cl = 0;  // next chunk the X stream will load
    // small-K mode (encoders: K = 3 or 6 spatial coordinates): one zero-padded chunk, assembled
    // from scalar loads because a 12-byte row is not 16-byte addressable
    const bool smallk = a.K1_real < a.K1;  // wave-uniform
    auto small_x = [&]() -> f32x4 {
        const float* r0 = q0 - g * 4;
        const float* r1 = q1 - g * 4;
        const float* r2 = q2 - g * 4;
        const int w0 = a.seg_width[0], w1 = a.n_seg > 1 ? a.seg_width[1] : 0, w2 = a.n_seg > 2 ? a.seg_width[2] : 0;
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = g * 4 + r;
            float t = 0.f;
            if (k < w0) t = r0[k];
            else if (k < w0 + w1) t = r1[k - w0];
            else if (k < w0 + w1 + w2) t = r2[k - w0 - w1];
            v[r] = t;
        }
        return v;
    };
    auto next_x = [&](f32x4 fallback) -> f32x4 {
        f32x4 v = fallback;
        if (cl < nc && !smallk) v = *(const f32x4*)px;
        ++cl;
        px += 16;
        if (cl == c1) px = q1;
        if (cl == c2) px = q2;
        return v;
    };

    // ---------------- layer 1: K1 (runtime) -> NT1*16, weights through LDS, X from global
    f32x4 acc1[NT1];
    init_bias<NT1>(acc1, a.b[0], g);
    // pre-projected gathered segments: the row's accumulators start at b + sum_s P_s[idx_s[e]]
    // (this lane's 4 features of every 16-feature tile: 64-byte pieces of the 16 P rows per load)
    if (a.n_pre > 0) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (s < a.n_pre) {
                const long long r = (long long)a.pre_index[s][er];
                const float* p = a.pre_table[s] + (size_t)(r < 0 ? 0 : r) * (size_t)(NT1 * 16) + g * 4;
#pragma unroll
                for (int T = 0; T < NT1; ++T) {
                    const f32x4 v = *(const f32x4*)(p + T * 16);
                    acc1[T].x += v.x;
                    acc1[T].y += v.y;
                    acc1[T].z += v.z;
                    acc1[T].w += v.w;
                }
            }
        }
    }
    __builtin_amdgcn_s_setprio(2);
    {
        constexpr int BUF = NT1 * 256;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        stage_w<NT1 * 16, NW>(a.W[0], a.K1, 0, lds, wave, lane);
        const int n_pieces = pieces_of<NT1 * 16, NW>(wave);
        f32x4 x0 = smallk ? small_x() : next_x(zero);
        f32x4 x1 = next_x(zero);
        for (int c = 0; c < nc; ++c) {
            wait_dma();
            if (!(a.ablate & 4)) __syncthreads();
            const f32x4 x2 = next_x(zero);
            const float* wb = lds + (c & 1) * BUF + lane * 4;
            WStage st = begin_stage<NW>(a.W[0], a.K1, (c + 1) * 16, lds + ((c + 1) & 1) * BUF, wave, lane);
            mma_chunk<NT1, NT1 * 16, NW>(acc1, wb, x0, st, (c + 1 < nc && !(a.ablate & 2)) ? n_pieces : 0);
            x0 = x1;
            x1 = x2;
        }
    }
    // Priority outranks age in the SIMD's issue arbitration: a wave in its (dense, wait-free) VALU
    // epilogue would otherwise starve the co-resident workgroup's MFMA stream whenever it is the
    // older of the two.  Epilogues run at priority 0, MFMA loops at priority 2.
    __builtin_amdgcn_s_setprio(0);
    dump_pre<NT1, PAD>(acc1, a.save_pre[0], e, valid, g, PAD ? a.real[0] : NT1 * 16);
    if constexpr (NT2 == 0) {
        // single-layer launch (fp32 at latent 512: a 1024-wide hidden layer is 256 accumulators per lane, so the
        // layers of an MLP run as separate launches and the hidden rows make one trip through HBM)
        // PARTIAL: the layer is narrower than its zero-padded storage (504 of 512: the supernode encoder's last
        // layer at latent 512): statistics over the real width with the padded features masked out, real-width store
        // PAD (single layers between the grid widths, mlp_fused_square.hip): the same masked statistics over a.real[0]
        // features; dump (above), skip and store at the real row width
        if constexpr (PAD) {
            if (!(a.ablate & 1))
                layernorm_act<NT1, ACT_O, true, false, true>(acc1, a.lnw[0], a.lnb[0], a.act[0], a.eps, g, a.real[0]);
            store_out_pad<NT1>(acc1, a, e, valid, g);
            return;
        }
        if (!(a.ablate & 1))
            layernorm_act<NT1, ACT_O, true, false, PARTIAL>(acc1, a.lnw[0], a.lnb[0], a.act[0], a.eps, g,
                                                            PARTIAL ? a.n_out_real : NT1 * 16);
        store_out<NT1, PARTIAL>(acc1, a, e, valid, g);
        return;
    }
    if constexpr (PLAIN) {
        act_only<NT1>(acc1, a.act[0]);
    } else if (!(a.ablate & 1))
        layernorm_act<NT1, ACT_H, true, false, PAD>(acc1, a.lnw[0], a.lnb[0], a.act[0], a.eps, g,
                                                    PAD ? a.real[0] : NT1 * 16);
    __builtin_amdgcn_s_setprio(2);

    // ---------------- layer 2 (and 3): activations stay in registers
    f32x4 acc2[NT2 > 0 ? NT2 : 2];
    constexpr int N2 = NT2 > 0 ? NT2 : 2;   // (NT2 == 0 returned above; N2 only keeps the dead code well-formed)
    init_bias<N2>(acc2, a.b[1], g);
    dense_from_regs<NT1, N2, NW>(acc1, acc2, a.W[1], lds, wave, lane, a.ablate);
    __builtin_amdgcn_s_setprio(0);
    dump_pre<N2, PAD>(acc2, a.save_pre[1], e, valid, g, PAD ? a.real[1] : N2 * 16);
    if constexpr (PLAIN) {
        act_only<N2>(acc2, a.act[1]);
    } else if (!(a.ablate & 1))
        layernorm_act<N2, (NT3 == 0 ? ACT_O : ACT_H), !(PLAIN_LAST && NT3 == 0), (PARTIAL && NT3 == 0 && !PAD), PAD>(
            acc2, a.lnw[1], a.lnb[1], a.act[1], a.eps, g, PAD ? a.real[1] : (NT3 == 0 ? a.n_out_real : N2 * 16));
    if constexpr (NT3 == 0) {
        if constexpr (PAD) store_out_pad<N2>(acc2, a, e, valid, g);
        else store_out<N2, PARTIAL>(acc2, a, e, valid, g);
    } else {
        f32x4 acc3[NT3];
        init_bias<NT3>(acc3, a.b[2], g);
        __builtin_amdgcn_s_setprio(2);
        dense_from_regs<N2, NT3, NW>(acc2, acc3, a.W[2], lds, wave, lane, a.ablate);
        __builtin_amdgcn_s_setprio(0);
        dump_pre<NT3, PAD>(acc3, a.save_pre[2], e, valid, g, PAD ? a.real[2] : NT3 * 16);
        if constexpr (PLAIN) {
            if constexpr (!PLAIN_LAST) act_only<NT3>(acc3, a.act[2]);
        } else if (!(a.ablate & 1))
            layernorm_act<NT3, ACT_O, !PLAIN_LAST, (PARTIAL && !PAD), PAD>(acc3, a.lnw[2], a.lnb[2], a.act[2], a.eps, g,
                                                                           a.n_out_real);
        if constexpr (PAD && !PLAIN_LAST) store_out_pad<NT3>(acc3, a, e, valid, g);
        else store_out<NT3, PARTIAL>(acc3, a, e, valid, g);
    }
}

template <int NT1, int NT2, int NT3, int MINW, int ACT_H, int ACT_O, bool PLAIN_LAST = false, int NW = 4,
          bool PARTIAL = false, bool PAD = false, bool PLAIN = false>
static int launch_mlp_act(const MlpArgs& a, hipStream_t s) {
    constexpr int maxnt = NT1 > NT2 ? (NT1 > NT3 ? NT1 : NT3) : (NT2 > NT3 ? NT2 : NT3);
    const size_t lds_bytes = (size_t)2 * maxnt * 256 * sizeof(float);
    const unsigned grid = (unsigned)ceil_div(a.M, NW * 16);
    auto kern = k_fused_mlp<NT1, NT2, NT3, MINW, ACT_H, ACT_O, PLAIN_LAST, NW, PARTIAL, PAD, PLAIN>;
    if (lds_bytes > 64 * 1024) {
        HGNN_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)lds_bytes));
    }
    kern<<<grid, NW * 64, lds_bytes, s>>>(a);
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}

// encoders whose output is narrower than their last tile row (supernode encoder: L - emb_dim,
// BipartiteClassification/Models/HGNN_GMM.py:117): LayerNorm + activation over the real width
template <int NT1, int NT2, int NT3, int MINW>
static int launch_mlp_partial(const MlpArgs& a, hipStream_t s) {
    const int n = NT3 == 0 ? 2 : 3;
    bool gelu = true;
    for (int l = 0; l < n; ++l) gelu = gelu && a.act[l] == HGNN_ACT_GELU;
    if (gelu) return launch_mlp_act<NT1, NT2, NT3, MINW, HGNN_ACT_GELU, HGNN_ACT_GELU, false, 4, true>(a, s);
    return launch_mlp_act<NT1, NT2, NT3, MINW, -1, -1, false, 4, true>(a, s);
}

template <int NT1, int NT2, int NT3, int MINW>
static int launch_mlp(const MlpArgs& a, hipStream_t s) {
    const int n = NT3 == 0 ? 2 : 3;
    bool hidden_gelu = true;
    for (int l = 0; l + 1 < n; ++l) hidden_gelu = hidden_gelu && a.act[l] == HGNN_ACT_GELU;
    const int out = a.act[n - 1];
    if (g_opt_mlp_act_switch) return launch_mlp_act<NT1, NT2, NT3, MINW, -1, -1>(a, s);
    // (round-2 null result, removed: 8 waves = 128 rows per workgroup, one workgroup per CU -- bitwise equal,
    // 3.6 % slower: one phase-locked workgroup does not overlap its epilogue with another's MFMAs)
    if (hidden_gelu && out == HGNN_ACT_TANH) return launch_mlp_act<NT1, NT2, NT3, MINW, HGNN_ACT_GELU, HGNN_ACT_TANH>(a, s);
    if (hidden_gelu && out == HGNN_ACT_GELU) return launch_mlp_act<NT1, NT2, NT3, MINW, HGNN_ACT_GELU, HGNN_ACT_GELU>(a, s);
    // SiLU in GELU's place (hidden_activation: SiLU): the cell networks' two combinations, compile-time as well
    bool hidden_silu = true;
    for (int l = 0; l + 1 < n; ++l) hidden_silu = hidden_silu && a.act[l] == HGNN_ACT_SILU;
    if (hidden_silu && out == HGNN_ACT_TANH) return launch_mlp_act<NT1, NT2, NT3, MINW, HGNN_ACT_SILU, HGNN_ACT_TANH>(a, s);
    if (hidden_silu && out == HGNN_ACT_SILU) return launch_mlp_act<NT1, NT2, NT3, MINW, HGNN_ACT_SILU, HGNN_ACT_SILU>(a, s);
    return launch_mlp_act<NT1, NT2, NT3, MINW, -1, -1>(a, s);
}

// one Linear -> LayerNorm -> act (+ skip) layer: the pieces of an fp32 MLP at latent 512
template <int NT1, int MINW, bool PARTIAL = false>
static int launch_single(const MlpArgs& a, hipStream_t s) {
    switch (a.act[0]) {
        case HGNN_ACT_GELU: return launch_mlp_act<NT1, 0, 0, MINW, HGNN_ACT_GELU, HGNN_ACT_GELU, false, 4, PARTIAL>(a, s);
        case HGNN_ACT_TANH: return launch_mlp_act<NT1, 0, 0, MINW, HGNN_ACT_TANH, HGNN_ACT_TANH, false, 4, PARTIAL>(a, s);
    }
    return launch_mlp_act<NT1, 0, 0, MINW, -1, -1, false, 4, PARTIAL>(a, s);
}

// heads: K -> H -> H -> w with a PLAIN last layer of w <= 32 real outputs (padded to 32 rows): the width-1
// classifiers (IN.py:107-115, HGNN_GMM.py:313-321) and the emb_dim-wide embedding head (HGNN_GMM.py:74-82);
// LayerNorm + act on the two hidden layers only
template <int NTH, int MINW>
static int launch_head(const MlpArgs& a, hipStream_t s) {
    if (a.act[0] == HGNN_ACT_GELU && a.act[1] == HGNN_ACT_GELU)
        return launch_mlp_act<NTH, NTH, 2, MINW, HGNN_ACT_GELU, HGNN_ACT_NONE, true, 4, true>(a, s);
    if (a.act[0] == HGNN_ACT_TANH && a.act[1] == HGNN_ACT_TANH)
        return launch_mlp_act<NTH, NTH, 2, MINW, HGNN_ACT_TANH, HGNN_ACT_NONE, true, 4, true>(a, s);
    return launch_mlp_act<NTH, NTH, 2, MINW, -1, HGNN_ACT_NONE, true, 4, true>(a, s);
}

// widths between the grid's (PAD kernels): the instantiation of the next grid width P, see hgnn_mlp_supported_f32_padded
template <int NT1, int NT2, int NT3, int MINW>
static int launch_mlp_pad(const MlpArgs& a, hipStream_t s) {
    const int n = NT3 == 0 ? 2 : 3;
    bool hidden_gelu = true;
    for (int l = 0; l + 1 < n; ++l) hidden_gelu = hidden_gelu && a.act[l] == HGNN_ACT_GELU;
    const int out = a.act[n - 1];
    if (hidden_gelu && out == HGNN_ACT_TANH)
        return launch_mlp_act<NT1, NT2, NT3, MINW, HGNN_ACT_GELU, HGNN_ACT_TANH, false, 4, false, true>(a, s);
    if (hidden_gelu && out == HGNN_ACT_GELU)
        return launch_mlp_act<NT1, NT2, NT3, MINW, HGNN_ACT_GELU, HGNN_ACT_GELU, false, 4, false, true>(a, s);
    return launch_mlp_act<NT1, NT2, NT3, MINW, -1, -1, false, 4, false, true>(a, s);
}

template <int NTH, int MINW>
static int launch_head_pad(const MlpArgs& a, hipStream_t s) {
    if (a.act[0] == HGNN_ACT_GELU && a.act[1] == HGNN_ACT_GELU)
        return launch_mlp_act<NTH, NTH, 2, MINW, HGNN_ACT_GELU, HGNN_ACT_NONE, true, 4, true, true>(a, s);
    return launch_mlp_act<NTH, NTH, 2, MINW, -1, HGNN_ACT_NONE, true, 4, true, true>(a, s);
}

}  // namespace hgnn
