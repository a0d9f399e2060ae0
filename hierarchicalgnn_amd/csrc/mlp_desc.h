// The hgnn_mlp_desc contract of the fused MLP entry points (include/hgnn_hip.h), host side, written once:
//   mlp_desc_shape_ok  what every hgnn_mlp_supported* checks before its own table of widths;
//   unpack_*           the pieces that copy a descriptor into a kernel-argument struct and check alignment.
// The four argument structs (MlpArgs, MlpArgsBf16, fs::Args, f3::Args) stay separate kernel arguments; each piece is a
// template over the struct and touches only the members it names, so a forward calls the pieces its struct has, in
// the order its checks have always run.  Element types and the row alignment (four elements: 16 bytes for fp32
// rows, 8 for bf16 rows) come from the struct's own pointer types.  ``fn`` is the entry point's name for messages.
#pragma once
#include <type_traits>
#include "common.h"

namespace hgnn {

// what one kernel accepts beyond its table of widths
struct MlpDescRules {
    int seg_multiple;            // every segment is a multiple of this many columns wide ...
    bool padded_storage;         // ... or K <= 16 as one zero-padded chunk (w0_cols = 16); w0_cols = K and any
                                 // w_last_rows pass on to the kernel's own table.  false: w0_cols = w_last_rows = 0
    int min_layers, max_layers;
    bool ln_everywhere;          // ln_w / ln_b on every layer (false: the kernel's own table says where)
    bool save_pre;               // save_pre[] may be set
    int max_pre;                 // n_pre in 0 .. max_pre
    bool m_int32;                // 0 <= M < 2^31 is part of the shape (false: the forward checks M)
};

inline bool mlp_desc_shape_ok(const hgnn_mlp_desc* d, const MlpDescRules& r) {
    if (d == nullptr) return false;
    if (d->n_seg < 1 || d->n_seg > 3 || d->n_layers < r.min_layers || d->n_layers > r.max_layers) return false;
    int k = 0;
    bool whole = true;
    for (int s = 0; s < d->n_seg; ++s) {
        if (d->seg_width[s] <= 0) return false;
        whole = whole && d->seg_width[s] % r.seg_multiple == 0;
        k += d->seg_width[s];
    }
    if (k != d->width[0]) return false;
    if (!r.padded_storage) {
        if (!whole || d->w0_cols != 0 || d->w_last_rows != 0) return false;
    } else if (!whole) {  // small-K mode: one zero-padded 16-column chunk
        if (k > 16 || d->w0_cols != 16) return false;
    } else if (d->w0_cols != 0 && d->w0_cols != k) {
        return false;
    }
    const int n = d->n_layers;
    for (int l = 0; l < n; ++l) {
        if (d->W[l] == nullptr || d->b[l] == nullptr) return false;
        if (r.ln_everywhere && (d->ln_w[l] == nullptr || d->ln_b[l] == nullptr)) return false;
    }
    if (!r.save_pre && (d->save_pre[0] || d->save_pre[1] || d->save_pre[2])) return false;
    if (d->n_pre < 0 || d->n_pre > r.max_pre) return false;
    for (int s = 0; s < d->n_pre; ++s)
        if (d->pre_table[s] == nullptr || d->pre_index[s] == nullptr) return false;
    if (r.m_int32 && (d->M < 0 || d->M > 0x7fffffffLL)) return false;
    return n != 3 || d->width[2] == d->width[1];
}

// a forward returns the first piece's refusal
#define HGNN_TRY(expr)                                                                \
    do {                                                                              \
        const int rc__ = (expr);                                                      \
        if (rc__ != HGNN_OK) return rc__;                                             \
    } while (0)

template <class P>
using mlp_ptr_t = std::remove_reference_t<P>;   // the type of a struct member, to cast the descriptor's pointer to
template <class A>
constexpr int mlp_row_align = 4 * (int)sizeof(*A().out);

inline bool mlp_aligned(const void* p, int bytes) { return (uintptr_t)p % (unsigned)bytes == 0; }

// segment tables, indices and widths; K1 (the columns stored per row of W[0]) and M.  Tables of either row type are
// 16-byte aligned
template <class A>
int unpack_segments(A& a, const hgnn_mlp_desc* d, const char* fn) {
    for (int s = 0; s < 3; ++s) {
        const bool on = s < d->n_seg;
        a.seg_table[s] = on ? (mlp_ptr_t<decltype(a.seg_table[s])>)d->seg_table[s] : nullptr;
        a.seg_index[s] = on ? d->seg_index[s] : nullptr;
        a.seg_width[s] = on ? d->seg_width[s] : 0;
        if (on) {
            HGNN_REQUIRE(a.seg_table[s] != nullptr && mlp_aligned(a.seg_table[s], 16),
                         "%s: segment table %d is NULL or not 16-byte aligned", fn, s);
        }
    }
    a.n_seg = d->n_seg;
    a.K1 = d->w0_cols != 0 ? d->w0_cols : d->width[0];
    a.M = d->M;
    return HGNN_OK;
}

// layer l's parameters and activation (slots past n_layers: NULL / 0) and the LayerNorm eps
template <class A>
int unpack_layer(A& a, const hgnn_mlp_desc* d, int l, const char* fn) {
    const bool on = l < d->n_layers;
    a.W[l] = on ? (mlp_ptr_t<decltype(a.W[l])>)d->W[l] : nullptr;
    a.b[l] = on ? d->b[l] : nullptr;
    a.lnw[l] = on ? d->ln_w[l] : nullptr;
    a.lnb[l] = on ? d->ln_b[l] : nullptr;
    a.act[l] = on ? d->act[l] : 0;
    a.eps = d->ln_eps;
    if (on) {
        HGNN_REQUIRE(mlp_aligned(a.W[l], 16) && mlp_aligned(a.b[l], 16) && mlp_aligned(a.lnw[l], 16) &&
                         mlp_aligned(a.lnb[l], 16),
                     "%s: layer %d parameters must be 16-byte aligned", fn, l);
    }
    if (on && a.lnw[l] == nullptr) a.lnw[l] = a.lnb[l] = a.b[l];  // never dereferenced (plain layer)
    return HGNN_OK;
}

// layer l's optional dump of its pre-LayerNorm rows
template <class A>
int unpack_save_pre(A& a, const hgnn_mlp_desc* d, int l, const char* fn) {
    a.save_pre[l] = l < d->n_layers ? (mlp_ptr_t<decltype(a.save_pre[l])>)d->save_pre[l] : nullptr;
    HGNN_REQUIRE(mlp_aligned(a.save_pre[l], mlp_row_align<A>), "%s: save_pre[%d] must be %d-byte aligned", fn, l,
                 mlp_row_align<A>);
    return HGNN_OK;
}

// the pre-projected gathered segments
template <class A>
int unpack_pre(A& a, const hgnn_mlp_desc* d, const char* fn) {
    a.n_pre = d->n_pre;
    for (int s = 0; s < 2; ++s) {
        a.pre_table[s] = s < d->n_pre ? (mlp_ptr_t<decltype(a.pre_table[s])>)d->pre_table[s] : nullptr;
        a.pre_index[s] = s < d->n_pre ? d->pre_index[s] : nullptr;
        HGNN_REQUIRE(mlp_aligned(a.pre_table[s], 16), "%s: pre_table[%d] must be 16-byte aligned", fn, s);
    }
    return HGNN_OK;
}

// the result and skip rows: every entry's last check
template <class A>
int unpack_out_skip(A& a, const hgnn_mlp_desc* d, void* out, const char* fn) {
    a.skip = (decltype(a.skip))d->skip;
    a.out = (decltype(a.out))out;
    HGNN_REQUIRE(mlp_aligned(out, mlp_row_align<A>) && mlp_aligned(a.skip, mlp_row_align<A>),
                 "%s: out/skip must be %d-byte aligned", fn, mlp_row_align<A>);
    return HGNN_OK;
}

}  // namespace hgnn
