// graph_intersection of the embedding stage (reference Modules/utils.py:117-166, scipy CSR on the host there).
//
// Output: every DISTINCT pred pair (row, col) in row-major order (what CSR -> COO gives), y = the pair also
// occurs in truth (c1*c2 - (c1 > c2) is never 0 when both have it and -1 when only pred has it; pairs only in
// truth are dropped), and with weights the sum of the truth weights over the truth copies of each output pair
// (0 when there are none).  Data flow (every array in the workspace):
//
//   pack     key = row << 31 | col, ids checked to lie in [0, 2^31) (a bad id sets the status, never faults)
//   pred     rocprim::radix_sort_keys (bits [0, 62)) -> rocprim::unique -> U distinct keys, count on the device
//   truth    rocprim::radix_sort_keys, or radix_sort_pairs (key, original position) with weights
//   emit     per distinct pred key: lower bound in the sorted truth keys -> y; the weight sum walks the run of
//            equal truth keys in their original order (the sort is stable): the only floating-point sum, fixed
//            order, so two calls give the same bits; unpack row / col
//
// The id range is not known on the host without a read, so the sorts cover the 62 bits of two 31-bit ids.
// Outputs are written at capacity e_pred, with out_count_and_status = {U, status}: the caller reads those two
// numbers once.
#include "common.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>

namespace hgnn {
namespace {

constexpr int kGiIdBits = 31;
constexpr unsigned kGiKeyBits = 2 * kGiIdBits;
constexpr uint64_t kGiIdMask = ((uint64_t)1 << kGiIdBits) - 1;

struct GiWorkspace {
    size_t pkey, pkey_s, ukey, count, tkey, tkey_s, tpos, tpos_s, err, temp, temp_bytes, total;
};

int gi_layout(int64_t ep, int64_t et, bool weights, GiWorkspace* w, hipStream_t stream) {
    size_t t1 = 0, t2 = 0, t3 = 0;
    if (ep > 0) {
        HGNN_CHECK_HIP(rocprim::radix_sort_keys(nullptr, t1, (uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)ep, 0u,
                                                kGiKeyBits, stream));
        HGNN_CHECK_HIP(rocprim::unique(nullptr, t2, (uint64_t*)nullptr, (uint64_t*)nullptr, (size_t*)nullptr,
                                       (size_t)ep, rocprim::equal_to<uint64_t>(), stream));
    }
    if (et > 0) {
        if (weights)
            HGNN_CHECK_HIP(rocprim::radix_sort_pairs(nullptr, t3, (uint64_t*)nullptr, (uint64_t*)nullptr,
                                                     (int32_t*)nullptr, (int32_t*)nullptr, (size_t)et, 0u, kGiKeyBits,
                                                     stream));
        else
            HGNN_CHECK_HIP(rocprim::radix_sort_keys(nullptr, t3, (uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)et,
                                                    0u, kGiKeyBits, stream));
    }
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    };
    const size_t p = (size_t)ep, t = (size_t)et;
    w->pkey = take(p * 8);
    w->pkey_s = take(p * 8);
    w->ukey = take(p * 8);
    w->count = take(sizeof(size_t));
    w->tkey = take(t * 8);
    w->tkey_s = take(t * 8);
    w->tpos = take(weights ? t * 4 : 0);
    w->tpos_s = take(weights ? t * 4 : 0);
    w->err = take(sizeof(int32_t));
    size_t tb = t1;
    for (size_t x : {t2, t3}) tb = x > tb ? x : tb;
    w->temp_bytes = tb;
    w->temp = take(tb + 256);
    w->total = off;
    return HGNN_OK;
}

unsigned gi_blocks(int64_t n) { return (unsigned)ceil_div(n > 0 ? n : 1, 256); }

// graph [2, E] int64 (rows, then cols) -> packed keys; pos (optional) = original position
__global__ __launch_bounds__(256) void k_gi_pack(const int64_t* __restrict__ g, int64_t E, uint64_t* __restrict__ key,
                                                 int32_t* __restrict__ pos, int32_t* __restrict__ err) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= E) return;
    int64_t r = g[i], c = g[E + i];
    const int64_t lim = (int64_t)1 << kGiIdBits;
    if (r < 0 || r >= lim || c < 0 || c >= lim) {
        atomicOr(err, 1);
        r = c = 0;
    }
    key[i] = ((uint64_t)r << kGiIdBits) | (uint64_t)c;
    if (pos != nullptr) pos[i] = (int32_t)i;
}

template <typename W>
__global__ __launch_bounds__(256) void k_gi_emit(const uint64_t* __restrict__ ukey, const size_t* __restrict__ count,
                                                 int64_t ep, const uint64_t* __restrict__ tkey, int64_t et,
                                                 const int32_t* __restrict__ tpos, const W* __restrict__ weights,
                                                 const int32_t* __restrict__ err, int64_t* __restrict__ out_graph,
                                                 uint8_t* __restrict__ out_y, W* __restrict__ out_w,
                                                 int64_t* __restrict__ out_cs) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t U = ep > 0 ? (int64_t)*count : 0;
    const int bad = *err;
    if (i == 0) {
        out_cs[0] = bad ? 0 : U;
        out_cs[1] = bad;
    }
    if (i >= U || bad) return;
    const uint64_t k = ukey[i];
    int64_t lo = 0, hi = et;   // first truth position with tkey >= k
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (tkey[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    out_graph[i] = (int64_t)(k >> kGiIdBits);
    out_graph[ep + i] = (int64_t)(k & kGiIdMask);
    out_y[i] = (lo < et && tkey[lo] == k) ? 1 : 0;
    if (out_w != nullptr) {
        W s = 0;
        for (int64_t j = lo; j < et && tkey[j] == k; ++j) s += weights[tpos[j]];
        out_w[i] = s;
    }
}

}  // namespace
}  // namespace hgnn

using namespace hgnn;

static int gi_check(const char* who, int64_t ep, int64_t et) {
    HGNN_REQUIRE(ep >= 0 && et >= 0, "%s: negative size", who);
    HGNN_REQUIRE(ep < ((int64_t)1 << 31) - 1 && et < ((int64_t)1 << 31) - 1, "%s: more than 2^31 - 2 pairs", who);
    return HGNN_OK;
}

extern "C" int hgnn_graph_intersection_workspace_bytes(int64_t e_pred, int64_t e_truth, int32_t with_weights,
                                                       size_t* bytes) {
    int rc = gi_check("hgnn_graph_intersection_workspace_bytes", e_pred, e_truth);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE(bytes != nullptr, "hgnn_graph_intersection_workspace_bytes: NULL bytes");
    GiWorkspace w;
    rc = gi_layout(e_pred, e_truth, with_weights != 0, &w, nullptr);
    if (rc != HGNN_OK) return rc;
    *bytes = w.total;
    return HGNN_OK;
}

extern "C" int hgnn_graph_intersection(const int64_t* pred, int64_t e_pred, const int64_t* truth, int64_t e_truth,
                                       const void* weights, int32_t weight_dtype, int64_t* out_graph, uint8_t* out_y,
                                       void* out_weights, int64_t* out_count_and_status, void* workspace,
                                       size_t workspace_bytes, hgnn_stream_t stream_) {
    const char* who = "hgnn_graph_intersection";
    hipStream_t stream = (hipStream_t)stream_;
    int rc = gi_check(who, e_pred, e_truth);
    if (rc != HGNN_OK) return rc;
    const bool with_w = weights != nullptr || out_weights != nullptr;
    HGNN_REQUIRE(out_count_and_status != nullptr, "%s: NULL out_count_and_status", who);
    HGNN_REQUIRE(e_pred == 0 || (pred != nullptr && out_graph != nullptr && out_y != nullptr), "%s: NULL pred array",
                 who);
    HGNN_REQUIRE(e_truth == 0 || truth != nullptr, "%s: NULL truth", who);
    HGNN_REQUIRE(!with_w || ((weights != nullptr || e_truth == 0) && (out_weights != nullptr || e_pred == 0)),
                 "%s: weights and out_weights go together", who);
    HGNN_REQUIRE(!with_w || weight_dtype == HGNN_DT_F32 || weight_dtype == HGNN_DT_F64,
                 "%s: weights must be float32 or float64 (dtype code %d)", who, weight_dtype);
    GiWorkspace w;
    rc = gi_layout(e_pred, e_truth, with_w, &w, stream);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE_WORKSPACE(who, workspace, workspace_bytes, w.total);
    char* ws = (char*)workspace;
    uint64_t *pkey = (uint64_t*)(ws + w.pkey), *pkey_s = (uint64_t*)(ws + w.pkey_s), *ukey = (uint64_t*)(ws + w.ukey);
    uint64_t *tkey = (uint64_t*)(ws + w.tkey), *tkey_s = (uint64_t*)(ws + w.tkey_s);
    int32_t *tpos = with_w ? (int32_t*)(ws + w.tpos) : nullptr, *tpos_s = with_w ? (int32_t*)(ws + w.tpos_s) : nullptr;
    size_t* count = (size_t*)(ws + w.count);
    int32_t* err = (int32_t*)(ws + w.err);
    void* temp = ws + w.temp;
    size_t tb = w.temp_bytes;

    HGNN_CHECK_HIP(hipMemsetAsync(err, 0, sizeof(int32_t), stream));
    if (e_truth > 0) {
        k_gi_pack<<<gi_blocks(e_truth), 256, 0, stream>>>(truth, e_truth, tkey, tpos, err);
        if (with_w)
            HGNN_CHECK_HIP(rocprim::radix_sort_pairs(temp, tb, tkey, tkey_s, tpos, tpos_s, (size_t)e_truth, 0u,
                                                     kGiKeyBits, stream));
        else
            HGNN_CHECK_HIP(rocprim::radix_sort_keys(temp, tb, tkey, tkey_s, (size_t)e_truth, 0u, kGiKeyBits, stream));
    }
    if (e_pred > 0) {
        k_gi_pack<<<gi_blocks(e_pred), 256, 0, stream>>>(pred, e_pred, pkey, nullptr, err);
        HGNN_CHECK_HIP(rocprim::radix_sort_keys(temp, tb, pkey, pkey_s, (size_t)e_pred, 0u, kGiKeyBits, stream));
        HGNN_CHECK_HIP(rocprim::unique(temp, tb, pkey_s, ukey, count, (size_t)e_pred, rocprim::equal_to<uint64_t>(),
                                       stream));
    }
    if (with_w && weight_dtype == HGNN_DT_F64)
        k_gi_emit<double><<<gi_blocks(e_pred), 256, 0, stream>>>(ukey, count, e_pred, tkey_s, e_truth, tpos_s,
                                                                 (const double*)weights, err, out_graph, out_y,
                                                                 (double*)out_weights, out_count_and_status);
    else
        k_gi_emit<float><<<gi_blocks(e_pred), 256, 0, stream>>>(ukey, count, e_pred, tkey_s, e_truth, tpos_s,
                                                                (const float*)weights, err, out_graph, out_y,
                                                                with_w ? (float*)out_weights : nullptr,
                                                                out_count_and_status);
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}
