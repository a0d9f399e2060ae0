// Square instantiations of the fused fp32 MLP kernel (mlp_fused_kernel.h, mapping described in mlp_fused.hip):
//     K -> h (-> h) -> h     the output as wide as the hidden layers (hidden_ratio 1, hidden == latent)
//     K -> h -> h -> o       h - 16 < o < h: the supernode encoder at hidden == latent
//     K -> h                 one Linear -> LayerNorm -> act (+ skip) below the 512 / 1024 of hgnn_mlp_forward_f32
// h a multiple of 16 in [32, 256].  h in {32, 64, 128, 256} with o == h runs on <h/16, h/16, 0 | h/16> as it is; every
// other shape on the PAD instantiation of the next grid width P >= h (zero-padded parameters, masked statistics, real
// row widths in HBM: layout in include/hgnn_hip.h, hgnn_mlp_supported_f32_square).  A translation unit of its own:
// the instantiations of mlp_fused.hip are untouched and the two compile side by side.
#include "mlp_fused_kernel.h"

using namespace hgnn;

// LayerNorm on every layer; 16-column chunks or small-K, padded storage; 1 to 3 layers
static const MlpDescRules kRulesF32Square = {/*seg_multiple*/ 16, /*padded_storage*/ true, /*layers*/ 1, 3,
                                             /*ln_everywhere*/ true, /*save_pre*/ true, /*max_pre*/ 2, /*m_int32*/ false};

// the grid width a square network of width h runs on: the smallest P of {32, 64, 128, 256} with P >= h (0: none)
static int square_grid(int h) {
    if (h < 32 || h > 256 || h % 16 != 0) return 0;
    for (int P = 32; P <= 256; P *= 2)
        if (P >= h) return P;
    return 0;
}

extern "C" int hgnn_mlp_supported_f32_square(const hgnn_mlp_desc* d) {
    if (!mlp_desc_shape_ok(d, kRulesF32Square)) return 0;
    const int n = d->n_layers;
    const int h = d->width[1];
    const int o = d->width[n];
    const int P = square_grid(h);
    if (P == 0) return 0;
    if (o == h) {
        // square / single: on the grid the parameters as they are, between the grid widths padded to P rows
        if (h == P) return (d->w_last_rows == 0 || d->w_last_rows == P) ? 1 : 0;
        return d->w_last_rows == P ? 1 : 0;
    }
    // K -> h -> h -> o with h - 16 < o < h real outputs: always the padded storage; inference only
    if (n != 3 || o <= h - 16 || o >= h || (o & 3) != 0 || d->w_last_rows != P || d->skip != nullptr) return 0;
    for (int l = 0; l < n; ++l)
        if (d->save_pre[l] != nullptr) return 0;
    return 1;
}

// single layers between the grid widths: launch_single's table on the PAD instantiation
template <int NT1, int MINW>
static int launch_single_pad(const MlpArgs& a, hipStream_t s) {
    switch (a.act[0]) {
        case HGNN_ACT_GELU: return launch_mlp_act<NT1, 0, 0, MINW, HGNN_ACT_GELU, HGNN_ACT_GELU, false, 4, false, true>(a, s);
        case HGNN_ACT_TANH: return launch_mlp_act<NT1, 0, 0, MINW, HGNN_ACT_TANH, HGNN_ACT_TANH, false, 4, false, true>(a, s);
    }
    return launch_mlp_act<NT1, 0, 0, MINW, -1, -1, false, 4, false, true>(a, s);
}

extern "C" int hgnn_mlp_forward_f32_square(const hgnn_mlp_desc* d, float* out, hgnn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    HGNN_REQUIRE(d != nullptr && out != nullptr, "hgnn_mlp_forward_f32_square: NULL argument");
    if (!hgnn_mlp_supported_f32_square(d)) {
        set_error("hgnn_mlp_forward_f32_square: unsupported shape (see hgnn_mlp_supported_f32_square in "
                  "include/hgnn_hip.h: K -> h (-> h) -> h, K -> h -> h -> o with h - 16 < o < h, or one layer K -> h, "
                  "LayerNorm everywhere, h a multiple of 16 in [32, 256], parameters zero padded to the next grid width)");
        return HGNN_ERR_UNSUPPORTED;
    }
    if (d->M == 0) return HGNN_OK;
    static const char fn[] = "hgnn_mlp_forward_f32_square";
    HGNN_REQUIRE(d->M > 0 && d->M < ((int64_t)1 << 31) * 64, "%s: bad M", fn);   // the grid (M / 64 workgroups) is 32 bits
    const int n = d->n_layers;
    MlpArgs a;
    HGNN_TRY(unpack_segments(a, d, fn));
    a.K1_real = d->width[0];
    a.n_out_real = d->width[n];
    for (int l = 0; l < 3; ++l) {
        HGNN_TRY(unpack_layer(a, d, l, fn));
        a.real[l] = l < n ? d->width[l + 1] : 0;
        HGNN_TRY(unpack_save_pre(a, d, l, fn));
    }
    a.ablate = g_opt_mlp_ablate;
    HGNN_TRY(unpack_pre(a, d, fn));
    HGNN_TRY(unpack_out_skip(a, d, out, fn));
    const int h = d->width[1];
    const int P = square_grid(h);
    const bool pad = h != P || d->width[n] != h;
    if (n == 1) {
        if (pad) {
            switch (P) {
                case 64: return launch_single_pad<4, 2>(a, stream);
                case 128: return launch_single_pad<8, 2>(a, stream);
                case 256: return launch_single_pad<16, 2>(a, stream);
            }
        } else {
            switch (P) {
                case 32: return launch_single<2, 2>(a, stream);
                case 64: return launch_single<4, 2>(a, stream);
                case 128: return launch_single<8, 2>(a, stream);
                case 256: return launch_single<16, 2>(a, stream);
            }
        }
    } else if (n == 2) {
        if (pad) {
            switch (P) {
                case 64: return launch_mlp_pad<4, 4, 0, 2>(a, stream);
                case 128: return launch_mlp_pad<8, 8, 0, 2>(a, stream);
                case 256: return launch_mlp_pad<16, 16, 0, 2>(a, stream);
            }
        } else {
            switch (P) {
                case 32: return launch_mlp<2, 2, 0, 2>(a, stream);
                case 64: return launch_mlp<4, 4, 0, 2>(a, stream);
                case 128: return launch_mlp<8, 8, 0, 2>(a, stream);
                case 256: return launch_mlp<16, 16, 0, 2>(a, stream);
            }
        }
    } else {
        if (pad) {   // P = 32: only the narrow last layer (h = 32 itself is on the grid)
            switch (P) {
                case 32: return launch_mlp_pad<2, 2, 2, 2>(a, stream);
                case 64: return launch_mlp_pad<4, 4, 4, 2>(a, stream);
                case 128: return launch_mlp_pad<8, 8, 8, 2>(a, stream);
                case 256: return launch_mlp_pad<16, 16, 16, 2>(a, stream);
            }
        } else {
            switch (P) {
                case 32: return launch_mlp<2, 2, 2, 2>(a, stream);
                case 64: return launch_mlp<4, 4, 4, 2>(a, stream);
                case 128: return launch_mlp<8, 8, 8, 2>(a, stream);
                case 256: return launch_mlp<16, 16, 16, 2>(a, stream);
            }
        }
    }
    set_error("hgnn_mlp_forward_f32_square: no instantiation");
    return HGNN_ERR_UNSUPPORTED;
}
