// Fused  gather -> concat -> [Linear -> LayerNorm -> act] x {2,3} -> (+skip)  on fp32 MFMA.
//
// Replaces, for one make_mlp Sequential (reference Modules/utils.py:169-196) and the
// concat/gather feeding it (Modules/gnn_utils.py:52-53, :61-62, :126, :134, :144, :152):
//     cat([nodes[g0], nodes[g1], edges]) -> Linear -> LN -> GELU -> Linear -> LN -> Tanh -> + edges
// without ever writing the [M,3L] concat, the gathered copies or the [M,H] hidden
// activations to HBM (>= 16 GB of avoidable traffic per cell at L=256, M=2M).
//
// Mapping (wave64, v_mfma_f32_16x16x4_f32, exact fp32 = fmaf chain):
//   * the GEMMs are evaluated TRANSPOSED:  D[f][e] = sum_k W[f][k] * X[e][k]
//     A operand = weight fragment, B operand = activations.  The D layout then
//     puts the edge on the lane (col = lane&15) and the features in registers
//     (row = 4*(lane>>4) + reg), so
//       - LayerNorm statistics over features are in-register sums plus two
//         cross-lane adds (no LDS, no cross-wave traffic);
//       - the activated accumulator tile of layer i IS the B operand of layer
//         i+1 (regs r=0..3 of tile c hold k = 16c + 4*(lane>>4) + r, exactly the
//         four k-steps of that tile) -- hidden activations never leave registers.
//   * one wave owns 16 edges and ALL features of every layer; a workgroup is 4
//     waves = 64 edges.  Weights stream through LDS in k-chunks of 16
//     (A-fragment order, filled by LDS-DMA global_load_lds_dwordx4, double
//     buffered, one barrier per chunk); the activations X are read straight from
//     global memory into the B-operand layout (16 rows x 64 B per wave load),
//     with the row gather folded into the per-lane address.
//   * 2 workgroups per CU (<=256 VGPRs); the 3-layer L=256 node network needs 320
//     accumulator registers and runs at 1 workgroup per CU.  NOTE: the fp32 MFMA
//     executes on the SIMD's fp32 vector ALUs, so epilogue VALU work does NOT hide
//     under a co-resident wave's MFMAs (measured): the epilogue is kept
//     short (branch-free erf/tanh) rather than overlapped.
//   * small-K mode (encoders, K = 3 / 6) and width-1 plain last layers (heads) are
//     handled by zero padding (see hgnn_mlp_desc in include/hgnn_hip.h); `save_pre`
//     dumps the pre-LayerNorm outputs for the opt-in differentiable variant.
//   * widths between the template grid's (PAD kernels, hgnn_mlp_forward_f32_padded): the next grid instantiation on
//     zero-padded parameters; LayerNorm statistics masked to the real features, dumps / skip / stores at the real
//     row widths.  PAD is false for every kernel of the native grid, whose device code does not depend on it.
#include "mlp_fused_kernel.h"

namespace hgnn {

int g_opt_mlp_act_switch = 0;   // hgnn_set_option("mlp_act_switch", 1): MEASUREMENT, every multi-layer fp32 launch takes the
                                // runtime-switch instantiation (ACT = -1) although its combination has one of its own
                                // (tools/bench_mlp_activations.py times the switch with it).  Same source arithmetic; the
                                // same bits on this file's kernels.  On the split-bf16 kernel the compiler may contract an
                                // inlined activation's last product into the hi / mid split that follows it: last-bit
                                // differences in the hidden planes, both inside the kernel's bar
int g_opt_mlp_ablate = 0;   // set through hgnn_set_option("mlp_ablate", bits): DIAGNOSTIC, wrong results

// the grid width a hidden width h runs on: the smallest P of {32, 64, 128, 256} with 2P >= h (0: none)
static int pad_grid(int h) {
    if (h < 32 || h > 512 || h % 16 != 0) return 0;
    for (int P = 32; P <= 256; P *= 2)
        if (2 * P >= h) return P;
    return 0;
}

// plain (no LayerNorm / activation) last layer of a 3-layer network = a head
static bool is_head(const hgnn_mlp_desc* d) { return d->n_layers == 3 && d->ln_w[2] == nullptr; }
// LayerNorm'ed last layer narrower than its zero-padded storage (supernode encoder)
static bool is_partial(const hgnn_mlp_desc* d) {
    return !is_head(d) && d->w_last_rows != 0 && d->w_last_rows != d->width[d->n_layers];
}

}  // namespace hgnn

using namespace hgnn;

// 16-column chunks or small-K, padded storage; LayerNorm-less last layers (heads) and M are checked below / in the forward
static const MlpDescRules kRulesF32 = {/*seg_multiple*/ 16, /*padded_storage*/ true, /*layers*/ 1, 3,
                                       /*ln_everywhere*/ false, /*save_pre*/ true, /*max_pre*/ 2, /*m_int32*/ false};
static const MlpDescRules kRulesF32Padded = {/*seg_multiple*/ 16, /*padded_storage*/ true, /*layers*/ 2, 3,
                                             /*ln_everywhere*/ false, /*save_pre*/ true, /*max_pre*/ 2, /*m_int32*/ false};

extern "C" int hgnn_mlp_supported(const hgnn_mlp_desc* d) {
    if (!mlp_desc_shape_ok(d, kRulesF32)) return 0;
    const int n = d->n_layers;
    const int h = d->width[1];
    const int o = d->width[n];
    if (n == 1) {
        // a single Linear -> LayerNorm -> act (+ skip) layer, 512 or 1024 wide: the building block of the fp32
        // MLPs at latent 512 (hidden 1024), which do not fit one launch; save_pre[0] dumps its pre-LayerNorm rows (the
        // first Linear of the encoders under autograd)
        if (d->ln_w[0] == nullptr || d->ln_b[0] == nullptr) return 0;
        if (d->w_last_rows != 0) {
            // narrower than its zero-padded storage of P = 512 rows (W, b, ln_w, ln_b): P - 16 < o < P, o % 4 == 0 (the
            // 504-wide last layer of the supernode encoder at latent 512); inference only
            const int P = d->w_last_rows;
            return (P == 512 && o > P - 16 && o < P && (o & 3) == 0 && d->skip == nullptr && d->save_pre[0] == nullptr) ? 1 : 0;
        }
        return (o == 512 || o == 1024) ? 1 : 0;
    }
    if (is_head(d)) {
        // K -> H -> H -> w (w <= 32): LayerNorm on the hidden layers only, plain last layer stored as 32 rows
        if (o < 1 || o > 32 || d->w_last_rows != 32 || d->act[2] != HGNN_ACT_NONE) return 0;
        if (d->ln_w[0] == nullptr || d->ln_b[0] == nullptr || d->ln_w[1] == nullptr || d->ln_b[1] == nullptr) return 0;
        if (d->skip != nullptr) return 0;
        return (h == 64 || h == 128 || h == 256 || h == 512) ? 1 : 0;
    }
    for (int l = 0; l < n; ++l)
        if (d->ln_w[l] == nullptr || d->ln_b[l] == nullptr) return 0;
    if (is_partial(d)) {
        // K -> 2P (-> 2P) -> o with o < P = w_last_rows real outputs, zero padded to P rows (W, b, ln_w, ln_b)
        const int P = d->w_last_rows;
        if (o < 4 || o >= P || (o & 3) != 0 || h != 2 * P || d->skip != nullptr) return 0;
        for (int l = 0; l < n; ++l)
            if (d->save_pre[l] != nullptr) return 0;
        return (n == 3 && (P == 32 || P == 64 || P == 128 || P == 256)) ? 1 : 0;
    }
    if (h != 2 * o) return 0;
    return (o == 32 || o == 64 || o == 128 || o == 256) ? 1 : 0;
}

extern "C" int hgnn_mlp_forward_f32(const hgnn_mlp_desc* d, float* out, hgnn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    HGNN_REQUIRE(d != nullptr && out != nullptr, "hgnn_mlp_forward_f32: NULL argument");
    if (!hgnn_mlp_supported(d)) {
        set_error("hgnn_mlp_forward_f32: unsupported shape (see hgnn_mlp_supported in include/hgnn_hip.h: "
                  "K -> 2L (-> 2L) -> L with LayerNorm everywhere, L in {32,64,128,256}, segments multiples "
                  "of 16 or K <= 16 zero-padded; or a K -> H -> H -> 1 head)");
        return HGNN_ERR_UNSUPPORTED;
    }
    if (d->M == 0) return HGNN_OK;
    static const char fn[] = "hgnn_mlp_forward_f32";
    HGNN_REQUIRE(d->M > 0 && d->M < ((int64_t)1 << 31) * 64, "%s: bad M", fn);   // the grid (M / 64 workgroups) is 32 bits
    MlpArgs a;
    HGNN_TRY(unpack_segments(a, d, fn));
    a.K1_real = d->width[0];
    a.n_out_real = d->width[d->n_layers];
    for (int l = 0; l < 3; ++l) HGNN_TRY(unpack_layer(a, d, l, fn));
    a.ablate = g_opt_mlp_ablate;
    for (int l = 0; l < 3; ++l) HGNN_TRY(unpack_save_pre(a, d, l, fn));
    // heads: the two LayerNorm'ed hidden layers can dump (training forward of the score heads); the plain last layer's
    // "pre-LayerNorm output" is the result itself
    HGNN_REQUIRE(!(is_head(d) && d->save_pre[2]), "%s: save_pre[2] is not available for heads", fn);
    HGNN_TRY(unpack_pre(a, d, fn));
    HGNN_TRY(unpack_out_skip(a, d, out, fn));
    if (is_head(d)) {
        switch (d->width[1]) {
            case 64: return launch_head<4, 2>(a, stream);
            case 128: return launch_head<8, 2>(a, stream);
            case 256: return launch_head<16, 2>(a, stream);
            case 512: return launch_head<32, 1>(a, stream);
        }
    }
    if (is_partial(d)) {
        switch (d->w_last_rows) {
            case 32: return launch_mlp_partial<4, 4, 2, 2>(a, stream);
            case 64: return launch_mlp_partial<8, 8, 4, 2>(a, stream);
            case 128: return launch_mlp_partial<16, 16, 8, 2>(a, stream);
            case 256: return launch_mlp_partial<32, 32, 16, 1>(a, stream);
        }
    }
    const int o = d->width[d->n_layers];
    if (d->n_layers == 1) {
        if (d->w_last_rows == 512 && o < 512) return launch_single<32, 2, true>(a, stream);
        switch (o) {
            case 512: return launch_single<32, 2>(a, stream);
            case 1024: return launch_single<64, 1>(a, stream);
        }
    }
    if (d->n_layers == 2) {
        switch (o) {
            case 32: return launch_mlp<4, 2, 0, 2>(a, stream);
            case 64: return launch_mlp<8, 4, 0, 2>(a, stream);
            case 128: return launch_mlp<16, 8, 0, 2>(a, stream);
            case 256: return launch_mlp<32, 16, 0, 2>(a, stream);
        }
    } else {
        switch (o) {
            case 32: return launch_mlp<4, 4, 2, 2>(a, stream);
            case 64: return launch_mlp<8, 8, 4, 2>(a, stream);
            case 128: return launch_mlp<16, 16, 8, 2>(a, stream);
            case 256: return launch_mlp<32, 32, 16, 1>(a, stream);
        }
    }
    set_error("hgnn_mlp_forward_f32: no instantiation");
    return HGNN_ERR_UNSUPPORTED;
}

// LayerNorm-less networks (make_mlp with layer_norm=False): the PLAIN kernels, activation codes read per layer
static bool plain_is_head(const hgnn_mlp_desc* d) {
    return d->n_layers == 3 && d->w_last_rows == 32 && d->width[3] <= 32 && d->act[2] == HGNN_ACT_NONE;
}

extern "C" int hgnn_mlp_supported_f32_plain(const hgnn_mlp_desc* d) {
    if (!mlp_desc_shape_ok(d, kRulesF32Padded)) return 0;   // 2 or 3 layers; segments, w0_cols, n_pre as for the grid kernels
    const int n = d->n_layers;
    const int h = d->width[1];
    const int o = d->width[n];
    for (int l = 0; l < n; ++l) {
        if (d->ln_w[l] != nullptr || d->ln_b[l] != nullptr) return 0;   // a mixed network is not this entry's
        if (d->act[l] < HGNN_ACT_NONE || d->act[l] > HGNN_ACT_LAST) return 0;
    }
    if (plain_is_head(d)) {
        // K -> H -> H -> w (w <= 32): the last layer a plain Linear stored as 32 rows
        if (o < 1 || d->skip != nullptr || d->save_pre[2] != nullptr) return 0;
        return (h == 64 || h == 128 || h == 256 || h == 512) ? 1 : 0;
    }
    if (d->w_last_rows != 0 && d->w_last_rows != o) {
        // K -> 2P -> 2P -> o with P - 16 < o < P real outputs, W / b of the last layer zero padded to P rows: without
        // statistics w_last_rows is only the store mask
        const int P = d->w_last_rows;
        if (n != 3 || o < 4 || o <= P - 16 || o >= P || (o & 3) != 0 || h != 2 * P || d->skip != nullptr) return 0;
        for (int l = 0; l < n; ++l)
            if (d->save_pre[l] != nullptr) return 0;
        return (P == 32 || P == 64 || P == 128 || P == 256) ? 1 : 0;
    }
    if (h != 2 * o) return 0;
    return (o == 32 || o == 64 || o == 128 || o == 256) ? 1 : 0;
}

template <int NT1, int NT2, int NT3, int MINW, bool PLAIN_LAST = false, bool PARTIAL = false>
static int launch_mlp_plain(const MlpArgs& a, hipStream_t s) {
    return launch_mlp_act<NT1, NT2, NT3, MINW, -1, -1, PLAIN_LAST, 4, PARTIAL, false, true>(a, s);
}

extern "C" int hgnn_mlp_forward_f32_plain(const hgnn_mlp_desc* d, float* out, hgnn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    HGNN_REQUIRE(d != nullptr && out != nullptr, "hgnn_mlp_forward_f32_plain: NULL argument");
    if (!hgnn_mlp_supported_f32_plain(d)) {
        set_error("hgnn_mlp_forward_f32_plain: unsupported shape (see hgnn_mlp_supported_f32_plain in "
                  "include/hgnn_hip.h: K -> 2L (-> 2L) -> L without LayerNorm on any layer, L in {32,64,128,256}, "
                  "segments multiples of 16 or K <= 16 zero-padded; or a K -> H -> H -> w head)");
        return HGNN_ERR_UNSUPPORTED;
    }
    if (d->M == 0) return HGNN_OK;
    static const char fn[] = "hgnn_mlp_forward_f32_plain";
    HGNN_REQUIRE(d->M > 0 && d->M < ((int64_t)1 << 31) * 64, "%s: bad M", fn);
    const int n = d->n_layers;
    MlpArgs a;
    HGNN_TRY(unpack_segments(a, d, fn));
    a.K1_real = d->width[0];
    a.n_out_real = d->width[n];
    for (int l = 0; l < 3; ++l) {
        HGNN_TRY(unpack_layer(a, d, l, fn));
        a.real[l] = 0;
        HGNN_TRY(unpack_save_pre(a, d, l, fn));
    }
    a.ablate = 0;
    HGNN_TRY(unpack_pre(a, d, fn));
    HGNN_TRY(unpack_out_skip(a, d, out, fn));
    if (plain_is_head(d)) {
        switch (d->width[1]) {
            case 64: return launch_mlp_plain<4, 4, 2, 2, true, true>(a, stream);
            case 128: return launch_mlp_plain<8, 8, 2, 2, true, true>(a, stream);
            case 256: return launch_mlp_plain<16, 16, 2, 2, true, true>(a, stream);
            case 512: return launch_mlp_plain<32, 32, 2, 1, true, true>(a, stream);
        }
    } else if (d->w_last_rows != 0 && d->w_last_rows != d->width[n]) {
        switch (d->w_last_rows) {
            case 32: return launch_mlp_plain<4, 4, 2, 2, false, true>(a, stream);
            case 64: return launch_mlp_plain<8, 8, 4, 2, false, true>(a, stream);
            case 128: return launch_mlp_plain<16, 16, 8, 2, false, true>(a, stream);
            case 256: return launch_mlp_plain<32, 32, 16, 1, false, true>(a, stream);
        }
    } else if (n == 2) {
        switch (d->width[n]) {
            case 32: return launch_mlp_plain<4, 2, 0, 2>(a, stream);
            case 64: return launch_mlp_plain<8, 4, 0, 2>(a, stream);
            case 128: return launch_mlp_plain<16, 8, 0, 2>(a, stream);
            case 256: return launch_mlp_plain<32, 16, 0, 2>(a, stream);
        }
    } else {
        switch (d->width[n]) {
            case 32: return launch_mlp_plain<4, 4, 2, 2>(a, stream);
            case 64: return launch_mlp_plain<8, 8, 4, 2>(a, stream);
            case 128: return launch_mlp_plain<16, 16, 8, 2>(a, stream);
            case 256: return launch_mlp_plain<32, 32, 16, 1>(a, stream);
        }
    }
    set_error("hgnn_mlp_forward_f32_plain: no instantiation");
    return HGNN_ERR_UNSUPPORTED;
}

extern "C" int hgnn_mlp_supported_f32_padded(const hgnn_mlp_desc* d) {
    if (!mlp_desc_shape_ok(d, kRulesF32Padded)) return 0;
    const int n = d->n_layers;
    const int h = d->width[1];
    const int o = d->width[n];
    const int P = pad_grid(h);
    if (P == 0) return 0;
    if (d->ln_w[0] == nullptr || d->ln_b[0] == nullptr || d->ln_w[1] == nullptr || d->ln_b[1] == nullptr) return 0;
    if (is_head(d)) {
        // K -> H -> H -> w (w <= 32): hidden layers stored 2P wide, the plain last layer as 32 rows of 2P columns
        if (o < 1 || o > 32 || d->w_last_rows != 32 || d->act[2] != HGNN_ACT_NONE) return 0;
        if (d->skip != nullptr || d->save_pre[2] != nullptr) return 0;
        return 1;
    }
    if (n == 3 && (d->ln_w[2] == nullptr || d->ln_b[2] == nullptr)) return 0;
    // K -> h (-> h) -> o: hidden layers stored 2P wide, the last layer as P rows
    if (o < 4 || (o & 3) != 0 || 2 * o > h || d->w_last_rows != P) return 0;
    return 1;
}

extern "C" int hgnn_mlp_forward_f32_padded(const hgnn_mlp_desc* d, float* out, hgnn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    HGNN_REQUIRE(d != nullptr && out != nullptr, "hgnn_mlp_forward_f32_padded: NULL argument");
    if (!hgnn_mlp_supported_f32_padded(d)) {
        set_error("hgnn_mlp_forward_f32_padded: unsupported shape (see hgnn_mlp_supported_f32_padded in "
                  "include/hgnn_hip.h: K -> h (-> h) -> o with LayerNorm everywhere, h a multiple of 16 in [32, 512], "
                  "o a multiple of 4 in [4, h / 2], parameters zero padded to the next grid width; or a "
                  "K -> H -> H -> w head)");
        return HGNN_ERR_UNSUPPORTED;
    }
    if (d->M == 0) return HGNN_OK;
    static const char fn[] = "hgnn_mlp_forward_f32_padded";
    HGNN_REQUIRE(d->M > 0 && d->M < ((int64_t)1 << 31) * 64, "%s: bad M", fn);
    const int n = d->n_layers;
    MlpArgs a;
    HGNN_TRY(unpack_segments(a, d, fn));
    a.K1_real = d->width[0];
    a.n_out_real = d->width[n];
    for (int l = 0; l < 3; ++l) {   // this entry has always checked each layer's dump right after its parameters
        HGNN_TRY(unpack_layer(a, d, l, fn));
        a.real[l] = l < n ? d->width[l + 1] : 0;
        HGNN_TRY(unpack_save_pre(a, d, l, fn));
    }
    a.ablate = g_opt_mlp_ablate;
    HGNN_TRY(unpack_pre(a, d, fn));
    HGNN_TRY(unpack_out_skip(a, d, out, fn));
    const int P = pad_grid(d->width[1]);
    if (is_head(d)) {
        switch (P) {
            case 32: return launch_head_pad<4, 2>(a, stream);
            case 64: return launch_head_pad<8, 2>(a, stream);
            case 128: return launch_head_pad<16, 2>(a, stream);
            case 256: return launch_head_pad<32, 1>(a, stream);
        }
    } else if (n == 2) {
        switch (P) {
            case 32: return launch_mlp_pad<4, 2, 0, 2>(a, stream);
            case 64: return launch_mlp_pad<8, 4, 0, 2>(a, stream);
            case 128: return launch_mlp_pad<16, 8, 0, 2>(a, stream);
            case 256: return launch_mlp_pad<32, 16, 0, 2>(a, stream);
        }
    } else {
        switch (P) {
            case 32: return launch_mlp_pad<4, 4, 2, 2>(a, stream);
            case 64: return launch_mlp_pad<8, 8, 4, 2>(a, stream);
            case 128: return launch_mlp_pad<16, 16, 8, 2>(a, stream);
            case 256: return launch_mlp_pad<32, 32, 16, 1>(a, stream);
        }
    }
    set_error("hgnn_mlp_forward_f32_padded: no instantiation");
    return HGNN_ERR_UNSUPPORTED;
}
