// k_wb_*: the pT-weighted binary cross-entropy of the training bases as one operator: the edge classifier's loss
// (reference EdgeClassifier/edge_classifier_base.py:99-111 get_training_weight, :127-128 the loss) and the assignment
// loss of BC-HGNN-GMM / gMRT after the matching (BipartiteClassification/bipartite_classification_base.py:123-138
// get_asgmt_weight, :189-190).  For pairs i with ids a_i in [0, NA), b_i in [0, NB) and scores s_i in [0, 1]:
//
//   raw_i = combine(ptw(pt_a[a_i]), ptw(pt_b[b_i]))      combine = sum (edge classifier) | max (assignment)
//   S_T = sum_{keep_i, y_i} raw_i                        S_F = sum_{keep_i, !y_i} raw_i
//   l_i = -(y_i ? max(log(s_i), -100) : max(log(1 - s_i), -100))       torch's binary_cross_entropy, 1 - s in float32
//   loss = sig(lwr) / S_T * sum_{keep, y} raw_i l_i  +  sig(-lwr) / S_F * sum_{keep, !y} raw_i l_i
//   dloss / ds_i = k_class(i) raw_i (s_i - y_i) / max((1 - s_i) s_i, 1e-12),  0 for a pair that is dropped or skipped
//
// Forward: ONE pass over the pairs (k_wb_forward) that accumulates the four sums in float64 -- per thread in a fixed
// order, per workgroup through a fixed tree -- and writes one partial per workgroup; k_wb_finish adds the partials in
// index order.  The grid is a function of P alone, so the bits are too: the tree, the grid and the id loader are
// det_reduce.h's.  The class normalisation is applied to the sums: no [P] weight vector exists.
// Backward: one elementwise pass (k_wb_backward) that recomputes raw_i and writes every element of grad_scores; no
// atomics, no plan.
// Streams per pair: the two ids, the score, y and keep (if given).  The pt tables stay cache-resident.
#include "common.h"
#include "det_reduce.h"
#include "ptw.h"
#include <cmath>
#include <type_traits>

namespace hgnn {
namespace {

constexpr int kWbAcc = 4;          // S_T, S_F, L_T, L_F

struct WbParams {
    float wmin, one_minus_wmin, leak, cut, cap, interval;   // pt_weighting (ptw_fill)
};

// raw_i, or false for a pair that takes no part: dropped by keep, or skipped with its status bit set in *bad
template <bool MAX>
__device__ __forceinline__ bool wb_pair(int64_t a, int64_t b, int64_t i, const float* __restrict__ scores,
                                        const uint8_t* __restrict__ keep, const float* __restrict__ pt_a, int64_t NA,
                                        const float* __restrict__ pt_b, int64_t NB, const WbParams& q, int* bad,
                                        float* s, float* raw) {
    if (keep != nullptr && keep[i] == 0) return false;
    if (a < 0 || a >= NA || b < 0 || b >= NB) {
        *bad |= HGNN_WB_ST_BAD_ID;
        return false;
    }
    const float v = scores[i];
    if (!(v >= 0.f && v <= 1.f)) {                           // NaN fails both comparisons
        *bad |= HGNN_WB_ST_BAD_SCORE;
        return false;
    }
    const float wa = ph_ptw(pt_a[a], q), wb = ph_ptw(pt_b[b], q);
    *raw = MAX ? ((wa > wb || wa != wa) ? wa : wb) : wa + wb;   // torch.maximum keeps NaN (interval == 0)
    *s = v;
    return true;
}

template <class IT, bool VEC_OK, bool MAX>
__global__ __launch_bounds__(kBlock) void k_wb_forward(const float* __restrict__ scores, const IT* __restrict__ ga,
                                                       const IT* __restrict__ gb, const uint8_t* __restrict__ y,
                                                       const uint8_t* __restrict__ keep,
                                                       const float* __restrict__ pt_a, int64_t NA,
                                                       const float* __restrict__ pt_b, int64_t NB, int64_t P,
                                                       WbParams q, double* __restrict__ partials,
                                                       int32_t* __restrict__ status) {
    constexpr int VEC = 16 / sizeof(IT);
    __shared__ double lds[kWavesPerBlock];
    double acc[kWbAcc] = {0.0, 0.0, 0.0, 0.0};
    const int64_t groups = (P + VEC - 1) / VEC;
    int bad = 0;
    for (int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x; g < groups; g += (int64_t)gridDim.x * kBlock) {
        const int64_t first = g * VEC;
        const int n = (int)(P - first < VEC ? P - first : VEC);
        int64_t a[VEC], b[VEC];
        load_pair_ids<IT, VEC_OK>(ga, first, n, a);
        load_pair_ids<IT, VEC_OK>(gb, first, n, b);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            if (j >= n) break;
            float s, raw;
            if (!wb_pair<MAX>(a[j], b[j], first + j, scores, keep, pt_a, NA, pt_b, NB, q, &bad, &s, &raw)) continue;
            const bool t = y[first + j] != 0;
            const float l = -fmaxf(logf(t ? s : 1.f - s), -100.f);
            const double r = (double)raw, rl = r * (double)l;
            acc[0] += t ? r : 0.0;
            acc[1] += t ? 0.0 : r;
            acc[2] += t ? rl : 0.0;
            acc[3] += t ? 0.0 : rl;
        }
    }
    if (bad) atomicOr(status, bad);
    for (int k = 0; k < kWbAcc; ++k) {                       // det_reduce.h write_partials: the same layout
        const double s = block_sum(acc[k], lds);
        if (threadIdx.x == 0) partials[(int64_t)k * gridDim.x + blockIdx.x] = s;
    }
}

// one workgroup: thread t adds partials t, t + 256, .. in that order, then the fixed tree.  state = {kT, kF, S_T, S_F,
// loss}: kT = sig(lwr) / S_T or 0 for a class without weight (the reference's 0/0 there; here it contributes nothing)
__global__ __launch_bounds__(kBlock) void k_wb_finish(const double* __restrict__ partials, int n_partials,
                                                      double sig_t, double sig_f, double* __restrict__ state,
                                                      float* __restrict__ loss) {
    __shared__ double lds[kWavesPerBlock];
    double tot[kWbAcc];
    for (int k = 0; k < kWbAcc; ++k) {                       // det_reduce.h total_partials: the same order
        double v = 0.0;
        for (int j = threadIdx.x; j < n_partials; j += kBlock) v += partials[(int64_t)k * n_partials + j];
        tot[k] = block_sum(v, lds);
    }
    if (threadIdx.x == 0) {
        const double kt = tot[0] > 0.0 ? sig_t / tot[0] : 0.0;
        const double kf = tot[1] > 0.0 ? sig_f / tot[1] : 0.0;
        const double l = kt * tot[2] + kf * tot[3];
        state[HGNN_WB_KT] = kt;
        state[HGNN_WB_KF] = kf;
        state[HGNN_WB_ST] = tot[0];
        state[HGNN_WB_SF] = tot[1];
        state[HGNN_WB_LOSS] = l;
        *loss = (float)l;
    }
}

// grad_i = g k_class raw_i (s_i - y_i) / max((1 - s_i) s_i, 1e-12): the quotient in float32 as torch's
// binary_cross_entropy backward forms it, the coefficient in float64, one rounding at the store
template <class IT, bool VEC_OK, bool MAX>
__global__ __launch_bounds__(kBlock) void k_wb_backward(const float* __restrict__ scores, const IT* __restrict__ ga,
                                                        const IT* __restrict__ gb, const uint8_t* __restrict__ y,
                                                        const uint8_t* __restrict__ keep,
                                                        const float* __restrict__ pt_a, int64_t NA,
                                                        const float* __restrict__ pt_b, int64_t NB, int64_t P,
                                                        WbParams q, const double* __restrict__ state,
                                                        const float* __restrict__ grad_out,
                                                        float* __restrict__ grad_scores) {
    constexpr int VEC = 16 / sizeof(IT);
    const double g0 = (double)grad_out[0];
    const double kt = g0 * state[HGNN_WB_KT], kf = g0 * state[HGNN_WB_KF];
    const int64_t groups = (P + VEC - 1) / VEC;
    int bad = 0;
    for (int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x; g < groups; g += (int64_t)gridDim.x * kBlock) {
        const int64_t first = g * VEC;
        const int n = (int)(P - first < VEC ? P - first : VEC);
        int64_t a[VEC], b[VEC];
        load_pair_ids<IT, VEC_OK>(ga, first, n, a);
        load_pair_ids<IT, VEC_OK>(gb, first, n, b);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            if (j >= n) break;
            float s, raw, c = 0.f;
            if (wb_pair<MAX>(a[j], b[j], first + j, scores, keep, pt_a, NA, pt_b, NB, q, &bad, &s, &raw)) {
                const bool t = y[first + j] != 0;
                const float quot = (s - (t ? 1.f : 0.f)) / fmaxf((1.f - s) * s, 1e-12f);
                c = (float)((t ? kt : kf) * (double)raw * (double)quot);
            }
            grad_scores[first + j] = c;
        }
    }
}

constexpr size_t kWbForwardBytes = (size_t)kWbAcc * kDetMaxGrid * sizeof(double);   // the partials

int wb_check(const char* what, const void* scores, const void* graph, int32_t index_dtype, const void* y,
             const void* pt_a, int64_t NA, const void* pt_b, int64_t NB, int64_t P, int32_t combine) {
    HGNN_REQUIRE(P >= 0 && NA >= 0 && NB >= 0, "%s: need P, NA, NB >= 0", what);
    HGNN_REQUIRE(index_dtype == HGNN_DT_I32 || index_dtype == HGNN_DT_I64, "%s: index_dtype must be I32 or I64", what);
    HGNN_REQUIRE(combine == HGNN_WB_COMBINE_SUM || combine == HGNN_WB_COMBINE_MAX,
                 "%s: combine must be HGNN_WB_COMBINE_SUM or HGNN_WB_COMBINE_MAX", what);
    HGNN_REQUIRE(P == 0 || (scores != nullptr && graph != nullptr && y != nullptr), "%s: NULL pointer", what);
    HGNN_REQUIRE((NA == 0 || pt_a != nullptr) && (NB == 0 || pt_b != nullptr), "%s: a pt table is NULL", what);
    return HGNN_OK;
}

WbParams wb_params(const double* h) {
    WbParams q;
    ptw_fill(q, h);
    return q;
}

// fn(index type tag, VEC_OK, MAX): the three compile-time choices of the per-pair kernels
template <class Fn>
void wb_dispatch(const void* graph, int64_t P, int32_t index_dtype, int32_t combine, Fn&& fn) {
    with_index_type(index_dtype, graph, P, [&](auto it, auto vk) {
        if (combine == HGNN_WB_COMBINE_MAX) fn(it, vk, std::true_type{});
        else fn(it, vk, std::false_type{});
    });
}

}  // namespace
}  // namespace hgnn

using namespace hgnn;

extern "C" int hgnn_weighted_bce_workspace_bytes(int64_t P, int32_t backward, size_t* bytes) {
    HGNN_REQUIRE(bytes != nullptr, "hgnn_weighted_bce_workspace_bytes: bytes is NULL");
    HGNN_REQUIRE(P >= 0, "hgnn_weighted_bce_workspace_bytes: need P >= 0");
    *bytes = backward ? 0 : kWbForwardBytes;
    return HGNN_OK;
}

extern "C" int hgnn_weighted_bce_forward(const float* scores, const void* graph, int32_t index_dtype, const uint8_t* y,
                                         const uint8_t* keep, const float* pt_a, int64_t NA, const float* pt_b,
                                         int64_t NB, int64_t P, int32_t combine, const double* hparams, float* loss,
                                         double* state, int32_t* status, void* workspace, size_t workspace_bytes,
                                         hgnn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = wb_check("hgnn_weighted_bce_forward", scores, graph, index_dtype, y, pt_a, NA, pt_b, NB, P, combine);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE(hparams && loss && state && status, "hgnn_weighted_bce_forward: NULL pointer");
    HGNN_REQUIRE_WORKSPACE("hgnn_weighted_bce_forward", workspace, workspace_bytes, kWbForwardBytes);
    double* partials = (double*)workspace;
    const WbParams q = wb_params(hparams);
    double sig_t, sig_f;
    class_sigmoids(hparams[HGNN_PH_LOG_WEIGHT_RATIO], &sig_t, &sig_f);
    HGNN_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), stream));
    int n_partials = 0;
    if (P > 0) {
        wb_dispatch(graph, P, index_dtype, combine, [&](auto it, auto vk, auto mx) {
            using IT = decltype(it);
            const unsigned grid = det_grid(ceil_div(P, 16 / sizeof(IT)));
            n_partials = (int)grid;
            k_wb_forward<IT, decltype(vk)::value, decltype(mx)::value><<<grid, kBlock, 0, stream>>>(
                scores, (const IT*)graph, (const IT*)graph + P, y, keep, pt_a, NA, pt_b, NB, P, q, partials, status);
        });
    }
    k_wb_finish<<<1, kBlock, 0, stream>>>(partials, n_partials, sig_t, sig_f, state, loss);
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}

extern "C" int hgnn_weighted_bce_backward(const float* scores, const void* graph, int32_t index_dtype,
                                          const uint8_t* y, const uint8_t* keep, const float* pt_a, int64_t NA,
                                          const float* pt_b, int64_t NB, int64_t P, int32_t combine,
                                          const double* hparams, const double* state, const float* grad_out,
                                          float* grad_scores, hgnn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = wb_check("hgnn_weighted_bce_backward", scores, graph, index_dtype, y, pt_a, NA, pt_b, NB, P, combine);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE(hparams && state && grad_out, "hgnn_weighted_bce_backward: NULL pointer");
    if (P == 0) return HGNN_OK;
    HGNN_REQUIRE(grad_scores != nullptr, "hgnn_weighted_bce_backward: NULL pointer");
    const WbParams q = wb_params(hparams);
    wb_dispatch(graph, P, index_dtype, combine, [&](auto it, auto vk, auto mx) {
        using IT = decltype(it);
        const unsigned grid = det_grid(ceil_div(P, 16 / sizeof(IT)));
        k_wb_backward<IT, decltype(vk)::value, decltype(mx)::value><<<grid, kBlock, 0, stream>>>(
            scores, (const IT*)graph, (const IT*)graph + P, y, keep, pt_a, NA, pt_b, NB, P, q, state, grad_out,
            grad_scores);
    });
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}
