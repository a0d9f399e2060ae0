// Host-side plumbing shared by the row kernels (segreduce.hip, segreduce_bf16.hip, segminmax.hip): the view of a
// plan's item list that a launch takes, the column count -> row shape dispatch, and grid sizing.
#pragma once
#include "common.h"
#include "options.h"
#include <type_traits>

namespace hgnn {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// One item list of a plan as the kernels take it (one wave per item), with the plan-level index arrays.
struct ItemView {
    const int32_t *begin, *end, *target;  // per item: its rows [begin, end) and where the result goes
    const int32_t* n_items;               // device-side count; max_items bounds it on the host
    int64_t max_items;
    const int32_t *src_row, *perm, *wi_dst;
};

// main pass: the plan's work items (one destination, or one chunk of a long list)
static inline ItemView work_items(const hgnn_plan* p) {
    return {p->wi_begin, p->wi_end, p->wi_target, p->counts + HGNN_CNT_WORK, p->max_work,
            p->src_row, p->perm, p->wi_dst};
}

// combine pass: split destination i sums the partial rows split_pbegin[i] .. split_pbegin[i + 1] - 1, read in
// place.  k_seg_window reads its item before the count is known, so `end` = split_pbegin + 1 needs max_split
// entries and split_pbegin therefore max_split + 1 (include/hgnn_hip.h, hgnn_plan).
static inline ItemView split_items(const hgnn_plan* p) {
    return {p->split_pbegin, p->split_pbegin + 1, p->split_dst, p->counts + HGNN_CNT_SPLIT, p->max_split,
            nullptr, nullptr, nullptr};
}

// What the fp32 sum kernels take on top of an item list (hgnn_segment_reduce_f32_ex).  `order` != NULL: the wave in
// slot i takes item order[i].  `arrive` != NULL: a chunk adds to arrive[s] after its partial row is out, and the
// chunk of split destination s that arrives last sums the rows split_pbegin[s] .. split_pbegin[s + 1] - 1 and
// writes out[split_dst[s]], so that no combine launch follows.  Both NULL: the two-launch kernels as they were.
struct ItemExtra {
    const int32_t* order;
    int32_t* arrive;
    const int32_t *split_pbegin, *split_dst, *n_split;
    int32_t max_split;
};

static inline ItemExtra item_extra(const hgnn_plan* p, const int32_t* order, int32_t* arrive) {
    return {order, arrive, p->split_pbegin, p->split_dst, p->counts + HGNN_CNT_SPLIT, (int32_t)p->max_split};
}

// Row shape of a row of `ncol` 16-byte columns: RL lanes per row (a power of two) and VPL loads per lane, handed
// to fn as compile-time constants: fn(integral_constant<int, RL>, integral_constant<int, VPL>).  MAX_COLS is the
// widest row the caller admits (256 columns of 4 floats, 64 columns of 8 bf16).  What else a kernel is
// instantiated with (rows in flight U, waves per workgroup WPB) is tuned per operation and stays next to it.
template <int MAX_COLS, class Fn>
static inline void for_row_shape(int ncol, Fn&& fn) {
    using std::integral_constant;
    constexpr integral_constant<int, 1> one{};
    if (ncol <= 4) fn(integral_constant<int, 4>{}, one);
    else if (ncol <= 8) fn(integral_constant<int, 8>{}, one);
    else if (ncol <= 16) fn(integral_constant<int, 16>{}, one);
    else if (ncol <= 32) fn(integral_constant<int, 32>{}, one);
    else if (MAX_COLS <= 64 || ncol <= 64) fn(integral_constant<int, 64>{}, one);
    else if constexpr (MAX_COLS > 64) {
        if (ncol <= 128) fn(integral_constant<int, 64>{}, integral_constant<int, 2>{});
        else fn(integral_constant<int, 64>{}, integral_constant<int, 4>{});
    }
}

// one wave per item, WPB waves per workgroup; nothing to launch for an empty list
template <int WPB, class... P, class... A>
static inline void launch_items(void (*kernel)(P...), int64_t max_items, hipStream_t s, A... args) {
    const unsigned grid = (unsigned)ceil_div(max_items, WPB);
    if (grid) kernel<<<grid, WPB * 64, 0, s>>>(args...);
}

// grid-strided kernels: at most 256 CUs x 8 blocks, x4 for balance, and never an empty grid
static inline unsigned capped_grid(int64_t blocks) {
    const int64_t cap = 256 * 8 * 4;
    return (unsigned)(blocks < 1 ? 1 : blocks > cap ? cap : blocks);
}
// ... with one 64-row tile per wave, kWavesPerBlock waves per workgroup
static inline unsigned stream_grid(int64_t n_tiles) { return capped_grid(ceil_div(n_tiles, kWavesPerBlock)); }

}  // namespace hgnn
