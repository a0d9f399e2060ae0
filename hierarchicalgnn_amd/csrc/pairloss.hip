// k_ph_*: the weighted squared pair hinge loss of the embedding stage (reference GNNEmbedding/embedding_base.py
// :95-107 pt_weighting, :137-146 get_training_weight, :148-155 get_hinge_distance, :167-168 the loss) as one operator.
//
//   raw_i = ptw(pt[a_i]) + ptw(pt[b_i])            S_T = sum_{y_i} raw_i      S_F = sum_{!y_i} raw_i
//   d_i   = sqrt(|E[a_i] - E[b_i]|^2 + 1e-12)      l_i = y_i ? scale d_i : max(0, margin - scale d_i)
//   loss  = sig(lwr) / S_T * sum_{y_i} raw_i l_i^2  +  sig(-lwr) / S_F * sum_{!y_i} raw_i l_i^2
//
// Forward: ONE pass over the pairs (k_ph_forward) that accumulates the four sums in float64 -- per thread in a fixed
// order, per workgroup through a fixed tree -- and writes one partial per workgroup; k_ph_finish adds the partials in
// index order.  The grid is a function of P alone, so the bits are too: the tree, the grid and the id loader are
// det_reduce.h's.  The class normalisation is applied to the sums, not to every pair: no second pass and no [P]
// weight vector.
// Backward: k_ph_coef writes one coefficient per pair; k_ph_grad walks the destination-sorted plan over cat(a, b)
// (gather index cat(b, a): every pair sits in the list of both endpoints) and sums  grad[v] = sum c_i (E[v] - E[o])
// over v's list in the plan's fixed order.  No floating-point atomics anywhere.
// Streams per pair: the two ids and y.  E (N x D floats) and pt stay cache-resident; nothing of shape [P, D] exists.
#include "common.h"
#include "det_reduce.h"
// ph_ptw(pt, params): pt_weighting in float32 with a NaN pt read as 0.  It lives in a header of its own because
// k_wb_* (wbce.hip, the weighted BCE) weighs the endpoints of its pairs with the same function.
#include "ptw.h"
#include <cmath>
#include <type_traits>

namespace hgnn {
namespace {

constexpr int kPhAcc = 4;          // S_T, S_F, L_T, L_F

struct PhParams {
    float wmin, one_minus_wmin, leak, cut, cap, interval;   // pt_weighting (ptw_fill)
    float margin, scale;
};

// |E[a] - E[b]|^2 is ONE chain s = fmaf(d_k, d_k, s) over k = 0 .. D - 1 on both paths, written out: left to the
// compiler's contraction, the float4 path became a mix of fused and packed unfused steps and the scalar path all
// fused, so the bits of the loss depended on the alignment of E.
template <bool V4>
__device__ __forceinline__ float ph_dist(const float* __restrict__ E, int64_t a, int64_t b, int D) {
    float s = 0.f;
    if constexpr (V4) {
        const float4* pa = reinterpret_cast<const float4*>(E + a * D);
        const float4* pb = reinterpret_cast<const float4*>(E + b * D);
        for (int k = 0; k < D / 4; ++k) {
            const float4 u = pa[k], v = pb[k];
            const float d0 = u.x - v.x, d1 = u.y - v.y, d2 = u.z - v.z, d3 = u.w - v.w;
            s = fmaf(d0, d0, s);
            s = fmaf(d1, d1, s);
            s = fmaf(d2, d2, s);
            s = fmaf(d3, d3, s);
        }
    } else {
        for (int k = 0; k < D; ++k) {
            const float d = E[a * D + k] - E[b * D + k];
            s = fmaf(d, d, s);
        }
    }
    return sqrtf(s + 1e-12f);
}

template <class IT, bool VEC_OK, bool V4>
__global__ __launch_bounds__(kBlock) void k_ph_forward(const float* __restrict__ E, int64_t N, int D,
                                                       const IT* __restrict__ ga, const IT* __restrict__ gb,
                                                       const uint8_t* __restrict__ y, const float* __restrict__ pt,
                                                       int64_t P, PhParams q, double* __restrict__ partials,
                                                       int32_t* __restrict__ status) {
    constexpr int VEC = 16 / sizeof(IT);
    __shared__ double lds[kWavesPerBlock];
    double acc[kPhAcc] = {0.0, 0.0, 0.0, 0.0};
    const int64_t groups = (P + VEC - 1) / VEC;
    bool bad = false;
    for (int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x; g < groups; g += (int64_t)gridDim.x * kBlock) {
        const int64_t first = g * VEC;
        const int n = (int)(P - first < VEC ? P - first : VEC);
        int64_t a[VEC], b[VEC];
        load_pair_ids<IT, VEC_OK>(ga, first, n, a);
        load_pair_ids<IT, VEC_OK>(gb, first, n, b);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            if (j >= n) break;
            if (a[j] < 0 || a[j] >= N || b[j] < 0 || b[j] >= N) {
                bad = true;
                continue;
            }
            const bool t = y[first + j] != 0;
            const float raw = ph_ptw(pt[a[j]], q) + ph_ptw(pt[b[j]], q);
            const float td = q.scale * ph_dist<V4>(E, a[j], b[j], D);
            const double l = t ? (double)td : fmax(0.0, (double)q.margin - (double)td);
            const double r = (double)raw, rl = r * l * l;
            acc[0] += t ? r : 0.0;
            acc[1] += t ? 0.0 : r;
            acc[2] += t ? rl : 0.0;
            acc[3] += t ? 0.0 : rl;
        }
    }
    if (bad) atomicOr(status, 1);
    for (int k = 0; k < kPhAcc; ++k) {                       // det_reduce.h write_partials: the same layout
        const double s = block_sum(acc[k], lds);
        if (threadIdx.x == 0) partials[(int64_t)k * gridDim.x + blockIdx.x] = s;
    }
}

// one workgroup: thread t adds partials t, t + 256, .. in that order, then the fixed tree.  state = {kT, kF, S_T, S_F,
// loss}: kT = sig(lwr) / S_T or 0 for a class without weight (the reference's 0/0 there; here it contributes nothing)
__global__ __launch_bounds__(kBlock) void k_ph_finish(const double* __restrict__ partials, int n_partials,
                                                      double sig_t, double sig_f, double* __restrict__ state,
                                                      float* __restrict__ loss) {
    __shared__ double lds[kWavesPerBlock];
    double tot[kPhAcc];
    for (int k = 0; k < kPhAcc; ++k) {                       // det_reduce.h total_partials: the same order
        double v = 0.0;
        for (int j = threadIdx.x; j < n_partials; j += kBlock) v += partials[(int64_t)k * n_partials + j];
        tot[k] = block_sum(v, lds);
    }
    if (threadIdx.x == 0) {
        const double kt = tot[0] > 0.0 ? sig_t / tot[0] : 0.0;
        const double kf = tot[1] > 0.0 ? sig_f / tot[1] : 0.0;
        const double l = kt * tot[2] + kf * tot[3];
        state[HGNN_PH_KT] = kt;
        state[HGNN_PH_KF] = kf;
        state[HGNN_PH_ST] = tot[0];
        state[HGNN_PH_SF] = tot[1];
        state[HGNN_PH_LOSS] = l;
        *loss = (float)l;
    }
}

// c_i = g * 2 w_i l_i (dl_i / dd_i) / d_i: the gradient of pair i is +-c_i (E[a_i] - E[b_i])
template <class IT, bool VEC_OK, bool V4>
__global__ __launch_bounds__(kBlock) void k_ph_coef(const float* __restrict__ E, int64_t N, int D,
                                                    const IT* __restrict__ ga, const IT* __restrict__ gb,
                                                    const uint8_t* __restrict__ y, const float* __restrict__ pt,
                                                    int64_t P, PhParams q, const double* __restrict__ state,
                                                    const float* __restrict__ grad_out, float* __restrict__ coef) {
    constexpr int VEC = 16 / sizeof(IT);
    const double g2 = 2.0 * (double)grad_out[0];
    const double kt = g2 * state[HGNN_PH_KT] * (double)q.scale * (double)q.scale;
    const double kf = -g2 * state[HGNN_PH_KF] * (double)q.scale;
    const int64_t groups = (P + VEC - 1) / VEC;
    for (int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x; g < groups; g += (int64_t)gridDim.x * kBlock) {
        const int64_t first = g * VEC;
        const int n = (int)(P - first < VEC ? P - first : VEC);
        int64_t a[VEC], b[VEC];
        load_pair_ids<IT, VEC_OK>(ga, first, n, a);
        load_pair_ids<IT, VEC_OK>(gb, first, n, b);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            if (j >= n) break;
            float c = 0.f;
            if (a[j] >= 0 && a[j] < N && b[j] >= 0 && b[j] < N) {
                const double raw = (double)(ph_ptw(pt[a[j]], q) + ph_ptw(pt[b[j]], q));
                if (y[first + j] != 0) {
                    c = (float)(kt * raw);                               // l = scale d: the 1 / d cancels
                } else {
                    const float d = ph_dist<V4>(E, a[j], b[j], D);
                    const double l = (double)q.margin - (double)(q.scale * d);
                    c = l > 0.0 ? (float)(kf * raw * l / (double)d) : 0.f;
                }
            }
            coef[first + j] = c;
        }
    }
}

// grad[v] = sum over the entries p of v's list of c_i (E[v] - E[other_p]), i the pair of entry p.  kPhLanes lanes share
// one destination: lane l adds the entries l, l + kPhLanes, .. of the list in that order, then a fixed xor tree; the
// list order is the plan's (stable by position in cat(a, b)), so the bits depend on neither the grid nor the chunk.
// The difference is formed before it is scaled, as autograd's backward of the reference expression does; each entry
// is one fmaf on both paths, so the bits do not depend on the alignment of E either.
constexpr int kPhLanes = 16;
template <bool V4>
__global__ __launch_bounds__(kBlock) void k_ph_grad(const float* __restrict__ E, int64_t N, int D,
                                                    const int32_t* __restrict__ rowptr,
                                                    const int32_t* __restrict__ perm,
                                                    const int32_t* __restrict__ other, int64_t P,
                                                    const float* __restrict__ coef, float* __restrict__ grad) {
    const int64_t v = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kPhLanes;
    const int lane = threadIdx.x % kPhLanes;
    const bool live = v < N;
    float mine[HGNN_PH_MAX_DIM], acc[HGNN_PH_MAX_DIM];
#pragma unroll
    for (int k = 0; k < HGNN_PH_MAX_DIM; ++k) {
        mine[k] = (live && k < D) ? E[v * D + k] : 0.f;
        acc[k] = 0.f;
    }
    const int d4 = D / 4;
    const int begin = live ? rowptr[v] : 0, end = live ? rowptr[v + 1] : 0;
    for (int p = begin + lane; p < end; p += kPhLanes) {
        const int32_t e = perm[p];
        const float c = coef[e < P ? e : e - P];
        const int64_t o = other[p];
        if (c == 0.f || o == v) continue;
        if constexpr (V4) {
            const float4* row = reinterpret_cast<const float4*>(E + o * D);   // D % 4 == 0, E 16-byte aligned
#pragma unroll
            for (int k = 0; k < HGNN_PH_MAX_DIM / 4; ++k) {
                if (k < d4) {
                    const float4 u = row[k];
                    acc[4 * k + 0] = fmaf(c, mine[4 * k + 0] - u.x, acc[4 * k + 0]);
                    acc[4 * k + 1] = fmaf(c, mine[4 * k + 1] - u.y, acc[4 * k + 1]);
                    acc[4 * k + 2] = fmaf(c, mine[4 * k + 2] - u.z, acc[4 * k + 2]);
                    acc[4 * k + 3] = fmaf(c, mine[4 * k + 3] - u.w, acc[4 * k + 3]);
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < HGNN_PH_MAX_DIM; ++k)
                if (k < D) acc[k] = fmaf(c, mine[k] - E[o * D + k], acc[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < HGNN_PH_MAX_DIM; ++k) {
#pragma unroll
        for (int off = kPhLanes / 2; off > 0; off >>= 1) acc[k] += __shfl_xor(acc[k], off);
        if (live && lane == 0 && k < D) grad[v * D + k] = acc[k];
    }
}

struct PhScratch {
    size_t partials, coef, total;
};

void ph_layout(int64_t P, int backward, PhScratch* s) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    };
    s->partials = take((size_t)kPhAcc * kDetMaxGrid * sizeof(double));
    s->coef = backward ? take((size_t)P * sizeof(float)) : 0;
    s->total = off;
}

int ph_check(const char* what, const void* E, int64_t N, int32_t D, const void* graph, int32_t index_dtype,
             const void* y, const void* pt, int64_t P) {
    HGNN_REQUIRE(N >= 0 && P >= 0 && D >= 1 && D <= HGNN_PH_MAX_DIM, "%s: need N, P >= 0 and 1 <= D <= %d (D = %d)",
                 what, HGNN_PH_MAX_DIM, D);
    HGNN_REQUIRE(2 * P < ((int64_t)1 << 31) - 1024 && N < ((int64_t)1 << 31) - 1024, "%s: sizes must fit int32", what);
    HGNN_REQUIRE(index_dtype == HGNN_DT_I32 || index_dtype == HGNN_DT_I64, "%s: index_dtype must be I32 or I64", what);
    HGNN_REQUIRE(P == 0 || (graph != nullptr && y != nullptr && E != nullptr && pt != nullptr), "%s: NULL pointer", what);
    return HGNN_OK;
}

PhParams ph_params(const double* h) {
    PhParams q;
    ptw_fill(q, h);
    q.margin = (float)h[HGNN_PH_MARGIN];
    q.scale = (float)h[HGNN_PH_SCALE];
    return q;
}

// fn(index type tag, VEC_OK, V4): the three compile-time choices of the per-pair kernels
template <class Fn>
void ph_dispatch(const void* E, int D, const void* graph, int64_t P, int32_t index_dtype, Fn&& fn) {
    const bool v4 = D % 4 == 0 && (uintptr_t)E % 16 == 0;
    with_index_type(index_dtype, graph, P, [&](auto it, auto vk) {
        if (v4) fn(it, vk, std::true_type{});
        else fn(it, vk, std::false_type{});
    });
}

}  // namespace
}  // namespace hgnn

using namespace hgnn;

extern "C" int hgnn_pair_hinge_workspace_bytes(int64_t P, int64_t N, int32_t D, int32_t backward, size_t* bytes) {
    HGNN_REQUIRE(bytes != nullptr, "hgnn_pair_hinge_workspace_bytes: bytes is NULL");
    HGNN_REQUIRE(N >= 0 && P >= 0 && D >= 1 && D <= HGNN_PH_MAX_DIM,
                 "hgnn_pair_hinge_workspace_bytes: need N, P >= 0 and 1 <= D <= %d", HGNN_PH_MAX_DIM);
    PhScratch s;
    ph_layout(P, backward, &s);
    *bytes = s.total;
    return HGNN_OK;
}

extern "C" int hgnn_pair_hinge_forward(const float* E, int64_t N, int32_t D, const void* graph, int32_t index_dtype,
                                       const uint8_t* y, const float* pt, int64_t P, const double* hparams,
                                       float* loss, double* state, int32_t* status, void* workspace,
                                       size_t workspace_bytes, hgnn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = ph_check("hgnn_pair_hinge_forward", E, N, D, graph, index_dtype, y, pt, P);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE(hparams && loss && state && status, "hgnn_pair_hinge_forward: NULL pointer");
    PhScratch s;
    ph_layout(P, 0, &s);
    HGNN_REQUIRE_WORKSPACE("hgnn_pair_hinge_forward", workspace, workspace_bytes, s.total);
    double* partials = (double*)((char*)workspace + s.partials);
    const PhParams q = ph_params(hparams);
    double sig_t, sig_f;
    class_sigmoids(hparams[HGNN_PH_LOG_WEIGHT_RATIO], &sig_t, &sig_f);
    HGNN_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), stream));
    int n_partials = 0;
    if (P > 0) {
        ph_dispatch(E, D, graph, P, index_dtype, [&](auto it, auto vk, auto v4) {
            using IT = decltype(it);
            const unsigned grid = det_grid(ceil_div(P, 16 / sizeof(IT)));
            n_partials = (int)grid;
            k_ph_forward<IT, decltype(vk)::value, decltype(v4)::value><<<grid, kBlock, 0, stream>>>(
                E, N, D, (const IT*)graph, (const IT*)graph + P, y, pt, P, q, partials, status);
        });
    }
    k_ph_finish<<<1, kBlock, 0, stream>>>(partials, n_partials, sig_t, sig_f, state, loss);
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}

extern "C" int hgnn_pair_hinge_backward(const hgnn_plan* plan, const float* E, int64_t N, int32_t D, const void* graph,
                                        int32_t index_dtype, const uint8_t* y, const float* pt, int64_t P,
                                        const double* hparams, const double* state, const float* grad_out,
                                        float* grad_E, void* workspace, size_t workspace_bytes,
                                        hgnn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = ph_check("hgnn_pair_hinge_backward", E, N, D, graph, index_dtype, y, pt, P);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE(hparams && state && grad_out, "hgnn_pair_hinge_backward: NULL pointer");
    if (N == 0) return HGNN_OK;
    HGNN_REQUIRE(grad_E != nullptr && E != nullptr, "hgnn_pair_hinge_backward: NULL pointer");
    if (P == 0) {
        HGNN_CHECK_HIP(hipMemsetAsync(grad_E, 0, (size_t)N * D * sizeof(float), stream));
        return HGNN_OK;
    }
    HGNN_REQUIRE(plan != nullptr && plan->n_rows == 2 * P && plan->n_dst == N && plan->n_src == N && plan->has_gather,
                 "hgnn_pair_hinge_backward: plan must be the gather plan of cat(a, b) -> cat(b, a) over N rows");
    HGNN_REQUIRE(plan->rowptr && plan->perm && plan->src_row, "hgnn_pair_hinge_backward: a plan array is NULL");
    PhScratch s;
    ph_layout(P, 1, &s);
    HGNN_REQUIRE_WORKSPACE("hgnn_pair_hinge_backward", workspace, workspace_bytes, s.total);
    float* coef = (float*)((char*)workspace + s.coef);
    const PhParams q = ph_params(hparams);
    ph_dispatch(E, D, graph, P, index_dtype, [&](auto it, auto vk, auto v4) {
        using IT = decltype(it);
        const unsigned grid = det_grid(ceil_div(P, 16 / sizeof(IT)));
        k_ph_coef<IT, decltype(vk)::value, decltype(v4)::value><<<grid, kBlock, 0, stream>>>(
            E, N, D, (const IT*)graph, (const IT*)graph + P, y, pt, P, q, state, grad_out, coef);
    });
    const unsigned grad_grid = (unsigned)ceil_div(N * kPhLanes, kBlock);
    if (D % 4 == 0 && (uintptr_t)E % 16 == 0)
        k_ph_grad<true><<<grad_grid, kBlock, 0, stream>>>(E, N, D, plan->rowptr, plan->perm, plan->src_row, P, coef,
                                                          grad_E);
    else
        k_ph_grad<false><<<grad_grid, kBlock, 0, stream>>>(E, N, D, plan->rowptr, plan->perm, plan->src_row, P, coef,
                                                           grad_E);
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}
