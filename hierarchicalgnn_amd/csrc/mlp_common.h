// Shared device helpers of the fused MLP kernels (fp32: mlp_fused.hip, bf16: mlp_fused_bf16.hip).
#pragma once
#include "common.h"

namespace hgnn {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Activations.  v_mfma_f32_16x16x4_f32 runs on the SIMD's fp32 vector ALUs (its rate IS the VALU FMA
// rate), so epilogue VALU work does not hide under a co-resident wave's MFMAs: every VALU
// instruction here is paid in full (ablation: LayerNorm+act were 15.7 % of the kernel with libm
// erff/tanhf).  Hence branch-free forms built on v_exp_f32 / v_rcp_f32:
//   erf : Abramowitz-Stegun 7.1.26, |abs error| <= 1.5e-7  (exact-GELU parity bar is 1e-4 rel)
//   tanh: 1 - 2/(exp(2|x|)+1), abs error ~1e-7
__device__ __forceinline__ float fast_erf(float x) {
    const float ax = __builtin_fabsf(x);
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.0f));
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    p *= t;
    const float e = __builtin_amdgcn_exp2f(-1.44269504088896341f * ax * ax);
    const float r = fmaf(-p, e, 1.0f);
    return __builtin_copysignf(r, x);
}

__device__ __forceinline__ float fast_tanh(float x) {
    const float ax = __builtin_fabsf(x);
    const float e = __builtin_amdgcn_exp2f(2.88539008177792681f * ax);  // exp(2|x|)
    const float r = fmaf(-2.0f, __builtin_amdgcn_rcpf(e + 1.0f), 1.0f);
    return __builtin_copysignf(r, x);
}

// SiLU, LeakyReLU, ELU, Sigmoid (HGNN_ACT_SILU .. HGNN_ACT_SIGMOID: the torch.nn classes at their constructor
// defaults).  u = 2^-24; v_exp_f32 and v_rcp_f32 are taken at 1 ulp (|rel| <= 2u); tests/act_ref.py emulates these
// forms in float32 and proves the bounds (tests/test_act_ref.py).
//   sigmoid(x)  = 1 / (1 + 2^(-x log2 e)): no cancellation at either end (x -> -inf: 2^(..) -> +inf, rcp -> 0;
//       x -> +inf: 1 / (1 + 0)).  The rounded exponent x log2 e costs 1.25 |x| u relative in the power (|x| u the
//       product's rounding, 0.22 |x| u the float32 constant), hence |rel error| <= (1.25 |x| + 6) u, |abs error| <= 4 u;
//       below x = -87 the result is 0 or denormal against a true value < 2^-125.
//   silu(x)     = x * sigmoid(x): |rel error| <= (1.25 |x| + 7) u, |abs error| <= 8 u.
//   sigmoid'(x) = e r^2 with e = 2^(-|x| log2 e) in (0, 1], r = 1 / (1 + e): the symmetric form, no 1 - s.
//       |rel error| <= (1.25 |x| + 9) u, |abs error| <= 3 u.
//   silu'(x)    = s + x e r^2, s = x >= 0 ? r : e r  (sigmoid from the same e, r): |abs error| <= 12 u on a value in
//       [-0.1, 1.1]; relative to max(|silu'|, 1/8): <= 64 u (silu' crosses zero at x = -1.2785).
//   leaky(x)    = x > 0 ? x : 0.01f x: one rounding; against the float64 slope 0.01 |rel error| <= 2 u (0.01f itself is
//       0.01 (1 + 2.2e-8)).  leaky' = x > 0 ? 1 : 0.01f.
//   elu(x)      = x > 0 ? x : expm1(x).  exp(x) - 1 cancels below |x| ~ 1: for -1/4 < x <= 0 it is the Taylor
//       polynomial x (1 + x/2 + x^2/6 + x^3/24 + x^4/120 + x^5/720) (truncation x^6/5040 <= 4.9e-8 relative at 1/4,
//       Horner rounding <= 3 u), else 2^(x log2 e) - 1, whose subtraction is exact for x <= -1/4 (Sterbenz or a result
//       in [-1, -1/2) with the power's own ulp) and inherits the power's absolute error <= (1.25 |x| + 2) u e^x <= 3 u:
//       |rel error| <= 16 u everywhere (worst at x = -1/4: 3 u e^-1/4 / (1 - e^-1/4) < 11 u), down to |x| = 2^-149.
//   elu'(x)     = x > 0 ? 1 : 2^(x log2 e): the power itself, never elu + 1 of a cancelled value; |rel error|
//       <= (1.25 |x| + 3) u (the power at 1 ulp off the correctly rounded value: 1.5 ulp = 3 u).
__device__ __forceinline__ float fast_sigmoid(float x) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504088896341f * x));
}

// sigmoid(x) and sigmoid'(x) from one v_exp_f32 and one v_rcp_f32 on the |x| side
__device__ __forceinline__ void sigmoid_val_grad(float x, float& s, float& ds) {
    const float e = __builtin_amdgcn_exp2f(-1.44269504088896341f * __builtin_fabsf(x));
    const float r = __builtin_amdgcn_rcpf(1.0f + e);
    const float er = e * r;
    s = x >= 0.f ? r : er;
    ds = er * r;
}

// expm1 of xn <= 0 given e = exp(xn)
__device__ __forceinline__ float elu_neg(float xn, float e) {
    float p = fmaf(1.0f / 720.0f, xn, 1.0f / 120.0f);
    p = fmaf(p, xn, 1.0f / 24.0f);
    p = fmaf(p, xn, 1.0f / 6.0f);
    p = fmaf(p, xn, 0.5f);
    p = fmaf(p, xn, 1.0f);
    return xn > -0.25f ? xn * p : e - 1.0f;
}

__device__ __forceinline__ float act_apply(float x, int act) {
    switch (act) {
        case HGNN_ACT_GELU: return 0.5f * x * (1.0f + fast_erf(x * 0.70710678118654752440f));
        case HGNN_ACT_TANH: return fast_tanh(x);
        case HGNN_ACT_RELU: return x > 0.f ? x : 0.f;
        case HGNN_ACT_SILU: return x * fast_sigmoid(x);
        case HGNN_ACT_LEAKY_RELU: return x > 0.f ? x : 0.01f * x;
        case HGNN_ACT_ELU: {
            const float xn = __builtin_fminf(x, 0.f);
            const float en = elu_neg(xn, __builtin_amdgcn_exp2f(1.44269504088896341f * xn));
            return x > 0.f ? x : en;
        }
        case HGNN_ACT_SIGMOID: return fast_sigmoid(x);
        default: return x;
    }
}

// exact-GELU derivative: Phi(y) + y * phi(y).  `a` = act(y) is read by Tanh only; the codes above ReLU take their
// derivative from y alone
__device__ __forceinline__ float act_grad(float y, float a, int act) {
    switch (act) {
        case HGNN_ACT_GELU: {
            const float cdf = 0.5f * (1.0f + fast_erf(y * 0.70710678118654752440f));
            const float pdf = 0.3989422804014327f * __builtin_amdgcn_exp2f(-0.72134752044448170368f * y * y);
            return fmaf(y, pdf, cdf);
        }
        case HGNN_ACT_TANH: return fmaf(-a, a, 1.0f);
        case HGNN_ACT_RELU: return y > 0.f ? 1.0f : 0.f;
        case HGNN_ACT_SILU: {
            float s, ds;
            sigmoid_val_grad(y, s, ds);
            return fmaf(y, ds, s);
        }
        case HGNN_ACT_LEAKY_RELU: return y > 0.f ? 1.0f : 0.01f;
        case HGNN_ACT_ELU: {
            const float e = __builtin_amdgcn_exp2f(1.44269504088896341f * __builtin_fminf(y, 0.f));
            return y > 0.f ? 1.0f : e;
        }
        case HGNN_ACT_SIGMOID: {
            float s, ds;
            sigmoid_val_grad(y, s, ds);
            return ds;
        }
        default: return 1.0f;
    }
}

// activation value and derivative from ONE evaluation of the transcendental part (act_apply + act_grad would
// evaluate the erf polynomial / exp twice)
__device__ __forceinline__ void act_val_grad(float y, int act, float& val, float& grad) {
    switch (act) {
        case HGNN_ACT_GELU: {
            // Phi(y) = 0.5 (1 + erf(y / sqrt 2)) by Abramowitz-Stegun 7.1.26 (as fast_erf), whose exp(-(y/sqrt 2)^2)
            // IS exp(-y^2 / 2), the Gaussian of the derivative's phi(y): one exp for both
            const float ax = __builtin_fabsf(y) * 0.70710678118654752440f;
            const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.0f));
            float p = fmaf(1.061405429f, t, -1.453152027f);
            p = fmaf(p, t, 1.421413741f);
            p = fmaf(p, t, -0.284496736f);
            p = fmaf(p, t, 0.254829592f);
            p *= t;
            const float e = __builtin_amdgcn_exp2f(-1.44269504088896341f * ax * ax);
            const float erf_abs = fmaf(-p, e, 1.0f);
            const float cdf = fmaf(0.5f, __builtin_copysignf(erf_abs, y), 0.5f);
            val = y * cdf;
            grad = fmaf(y, 0.3989422804014327f * e, cdf);
            return;
        }
        case HGNN_ACT_TANH: {
            const float t = fast_tanh(y);
            val = t;
            grad = fmaf(-t, t, 1.0f);
            return;
        }
        case HGNN_ACT_RELU:
            val = y > 0.f ? y : 0.f;
            grad = y > 0.f ? 1.0f : 0.f;
            return;
        case HGNN_ACT_SILU: {
            float s, ds;
            sigmoid_val_grad(y, s, ds);
            val = y * s;
            grad = fmaf(y, ds, s);
            return;
        }
        case HGNN_ACT_LEAKY_RELU:
            val = y > 0.f ? y : 0.01f * y;
            grad = y > 0.f ? 1.0f : 0.01f;
            return;
        case HGNN_ACT_ELU: {
            // one power: exp(min(y, 0)) is the derivative and feeds the value's far branch
            const float yn = __builtin_fminf(y, 0.f);
            const float e = __builtin_amdgcn_exp2f(1.44269504088896341f * yn);
            const float en = elu_neg(yn, e);
            val = y > 0.f ? y : en;
            grad = y > 0.f ? 1.0f : e;
            return;
        }
        case HGNN_ACT_SIGMOID:
            sigmoid_val_grad(y, val, grad);
            return;
        default:
            val = y;
            grad = 1.0f;
    }
}

// Weight staging.  W[NF][Kdim] row-major (torch Linear.weight); chunk = columns [k0, k0+16).
// One 1-KiB LDS-DMA piece covers 16 rows: lane (i = lane&15, g = lane>>4) fetches
// W[16p+i][k0+4g .. +3] and the DMA lands it at lane*16 bytes, i.e. the piece is stored in exactly
// the order the MFMA A-fragment read (ds_read_b128 at lane*16) wants: conflict-free, no swizzle.
// Address = wave-uniform piece base (SALU) + a fixed 32-bit per-lane byte offset.
// A tiny state machine so that only ONE per-lane 64-bit source pointer and one scalar LDS address
// stay live across the MFMA loop (eight precomputed piece addresses cost 16 VGPRs and pushed the
// L=256 kernel into scratch).
struct WStage {
    const char* src;        // per-lane source of the NEXT piece to issue
    unsigned lds;           // LDS byte address of the NEXT piece's destination (wave-uniform)
    unsigned piece_stride;  // bytes between this wave's consecutive pieces in W (64 rows)
};

__device__ __forceinline__ void wait_dma() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// Issued as inline asm on purpose: hipcc orders every later ds_read behind a builtin LDS-DMA with
// s_waitcnt vmcnt(0) (it cannot see that the DMA fills the OTHER buffer), which would serialise
// each piece's memory latency into the MFMA loop.  The hand-off is done by hand instead: every wave
// drains its DMAs (wait_dma) right before the barrier that publishes them.
__device__ __forceinline__ void dma_piece(const char* src, unsigned lds_addr) {
    asm volatile(
        "s_mov_b32 m0, %1\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %0, off"
        :
        : "v"(src), "s"(lds_addr)
        : "memory");  // m0 is a reserved register: hipcc re-materialises it before each of its own uses
}

__device__ __forceinline__ unsigned lds_addr_of(float* p) {
    return (unsigned)(size_t)(__attribute__((address_space(3))) float*)p;
}

// start staging one chunk (16 bytes per lane and row: 4 fp32 or 8 bf16 k-values per lane group) of a
// row-major weight matrix into `lds`: points at this wave's first piece
// (NW = waves per workgroup: piece p of a chunk is staged by wave p % NW)
template <int NW = 4>
__device__ __forceinline__ WStage begin_stage_bytes(const void* W, size_t row_bytes, size_t chunk_byte_off,
                                                    float* lds, int wave, int lane) {
    WStage st;
    st.src = (const char*)W + (size_t)(wave * 16 + (lane & 15)) * row_bytes + chunk_byte_off + (lane >> 4) * 16;
    st.lds = lds_addr_of(lds) + (unsigned)wave * 1024u;
    st.piece_stride = (unsigned)(NW * 16 * row_bytes);
    return st;
}

template <int NW = 4>
__device__ __forceinline__ WStage begin_stage(const float* W, int Kdim, int k0, float* lds, int wave, int lane) {
    return begin_stage_bytes<NW>(W, (size_t)Kdim * sizeof(float), (size_t)k0 * sizeof(float), lds, wave, lane);
}

template <int NW = 4>
__device__ __forceinline__ void stage_next(WStage& st) {
    dma_piece(st.src, st.lds);
    st.src += st.piece_stride;
    st.lds += NW * 1024u;  // NW pieces further
}

// number of pieces wave `wave` owns of an NF-row chunk (pieces p = wave, wave+NW, ...)
template <int NF, int NW = 4>
__device__ __forceinline__ int pieces_of(int wave) {
    constexpr int PIECES = NF / 16;
    return PIECES % NW == 0 ? PIECES / NW : (PIECES / NW + (wave < PIECES % NW ? 1 : 0));
}

}  // namespace hgnn
