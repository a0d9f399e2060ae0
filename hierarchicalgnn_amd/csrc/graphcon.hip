// k_gc_* / k_ga_*: what DynamicGraphConstruction (reference Modules/gnn_utils.py:171-218) does after the neighbour
// search, on the device.
//
// k_gc_*  edge lists from a kNN result idx int64 [nq, K] (ids in [0, n_pts), -1 = empty slot):
//   sym = 0   exclusive scan of the "valid" flags of the nq K slots in row-major order (rocprim::exclusive_scan over a
//             transform iterator: no flag array), then k_gc_fill writes (row, id) of every valid slot at its position.
//             This is torch.stack([ind[positive], idxs[positive]]).
//   sym = 1   k_gc_keys writes the keys (s << b | d) and (d << b | s) of every valid slot, b = ceil(log2 n), and the
//             marker 1 << 2b for an empty one; rocprim::radix_sort_keys over the 2b + 1 low bits, rocprim::unique,
//             k_gc_decode.  (s << b | d) orders the pairs as s n + d does, so this is symmetrize()'s graph.
//   The edge count and the status word go to one device int64[2]: the caller's single read.  An id >= n_pts or < -1
//   sets HGNN_GC_ST_BAD_ID; the slot is skipped and never used as an address.  The only atomic is an integer OR.
//
// k_ga_*  the attention weights of E edges as one operator:
//   x_e = <A[a_e], B[b_e]>                         (the arithmetic of hgnn_edge_dot_f32, lane for lane)
//   z_e = gamma (x_e - mu) rstd + beta             mu, var: the batch's (training) or the running ones (eval)
//   f_e = sigmoid(z_e) | exp(z_e),   w_e = f_e / (sum f / E) with norm, else f_e
//   Every sum (sum x, sum x^2, sum f; backward: sum g_w f, sum G, sum G xhat) is float64: per thread in a fixed order,
//   per workgroup through a fixed tree, one partial per workgroup, the partials added in index order
//   (det_reduce.h).  The grid depends on E alone, so the bits do too.  The elementwise part is float32 from the float64
//   scalars rounded once.  k_ga_stats also performs nn.BatchNorm1d's running-statistics update.
#include "common.h"
#include "det_reduce.h"
#include "rows_common.h"
#include <cmath>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include <type_traits>

namespace hgnn {
namespace {

// ------------------------------------------------------------------ k_gc
constexpr int64_t kGcMaxSlots = ((int64_t)1 << 30) - 1;   // nq K: positions are int32, sym doubles them

struct GcValid {
    int64_t n_pts;
    __host__ __device__ __forceinline__ int32_t operator()(const int64_t& v) const {
        return v >= 0 && v < n_pts ? 1 : 0;
    }
};

struct GcWorkspace {
    size_t pos, key, key_s, ukey, count, temp, temp_bytes, total;
};

int gc_bits(int64_t n) {
    int b = 0;
    while (((int64_t)1 << b) < n) ++b;
    return b;
}

// rocprim's scratch sizes are asked for once per shape and device: the wrapper calls hgnn_knn_edges_workspace_bytes
// and then hgnn_knn_edges with the same (slots, sym, bits), and a model repeats its shapes
int gc_layout(int64_t slots, int sym, int bits, GcWorkspace* w, hipStream_t stream) {
    thread_local int64_t last_slots = -1;
    thread_local int last_sym = 0, last_bits = 0, last_dev = -1;
    thread_local GcWorkspace last;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) dev = -1;           // no device: the size queries below report it
    if (dev >= 0 && dev == last_dev && slots == last_slots && sym == last_sym && bits == last_bits) {
        *w = last;
        return HGNN_OK;
    }
    size_t t1 = 0, t2 = 0;
    if (slots > 0) {
        if (sym) {
            HGNN_CHECK_HIP(rocprim::radix_sort_keys(nullptr, t1, (uint64_t*)nullptr, (uint64_t*)nullptr,
                                                    (size_t)(2 * slots), 0u, (unsigned)(2 * bits + 1), stream));
            HGNN_CHECK_HIP(rocprim::unique(nullptr, t2, (uint64_t*)nullptr, (uint64_t*)nullptr, (size_t*)nullptr,
                                           (size_t)(2 * slots), rocprim::equal_to<uint64_t>(), stream));
        } else {
            HGNN_CHECK_HIP(rocprim::exclusive_scan(
                nullptr, t1, rocprim::make_transform_iterator((const int64_t*)nullptr, GcValid{0}), (int32_t*)nullptr,
                (int32_t)0, (size_t)slots, rocprim::plus<int32_t>(), stream));
        }
    }
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    };
    const size_t s = (size_t)slots;
    w->pos = take(sym ? 0 : s * 4);
    w->key = take(sym ? 2 * s * 8 : 0);
    w->key_s = take(sym ? 2 * s * 8 : 0);
    w->ukey = take(sym ? 2 * s * 8 : 0);
    w->count = take(sizeof(size_t));
    w->temp_bytes = t1 > t2 ? t1 : t2;
    w->temp = take(w->temp_bytes + 256);
    w->total = off;
    last = *w;
    last_slots = slots;
    last_sym = sym;
    last_bits = bits;
    last_dev = dev;
    return HGNN_OK;
}

unsigned gc_blocks(int64_t n) { return (unsigned)ceil_div(n > 0 ? n : 1, kBlock); }

// one thread per slot; out = [2, cap]; the last slot's thread also writes the count
__global__ __launch_bounds__(kBlock) void k_gc_fill(const int64_t* __restrict__ idx, int64_t slots, int32_t K,
                                                    int64_t n_pts, const int32_t* __restrict__ pos, int64_t cap,
                                                    int64_t* __restrict__ out, int64_t* __restrict__ info) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= slots) return;
    const int64_t v = idx[i];
    const bool ok = v >= 0 && v < n_pts;
    const int64_t p = pos[i];
    if (ok && p < cap) {
        out[p] = i / K;
        out[cap + p] = v;
    }
    if (!ok && v != -1) atomicOr((unsigned long long*)(info + 1), (unsigned long long)HGNN_GC_ST_BAD_ID);
    if (i == slots - 1) info[0] = p + (ok ? 1 : 0);
}

__global__ __launch_bounds__(kBlock) void k_gc_keys(const int64_t* __restrict__ idx, int64_t slots, int32_t K,
                                                    int64_t n_pts, int bits, uint64_t* __restrict__ key,
                                                    int64_t* __restrict__ info) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= slots) return;
    const int64_t v = idx[i];
    const bool ok = v >= 0 && v < n_pts;
    const uint64_t s = (uint64_t)(i / K), d = (uint64_t)v, none = (uint64_t)1 << (2 * bits);
    key[2 * i] = ok ? (s << bits | d) : none;
    key[2 * i + 1] = ok ? (d << bits | s) : none;
    if (!ok && v != -1) atomicOr((unsigned long long*)(info + 1), (unsigned long long)HGNN_GC_ST_BAD_ID);
}

// the distinct keys ascending; the marker, if any slot was empty, is the last of them
__global__ __launch_bounds__(kBlock) void k_gc_decode(const uint64_t* __restrict__ ukey,
                                                      const size_t* __restrict__ n_unique, int bits, int64_t cap,
                                                      int64_t* __restrict__ out, int64_t* __restrict__ info) {
    const uint64_t none = (uint64_t)1 << (2 * bits), mask = ((uint64_t)1 << bits) - 1;
    int64_t n = (int64_t)*n_unique;
    if (n > cap) n = cap;
    if (n > 0 && ukey[n - 1] == none) --n;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) info[0] = n;
    if (i >= n) return;
    const uint64_t k = ukey[i];
    out[i] = (int64_t)(k >> bits);
    out[cap + i] = (int64_t)(k & mask);
}

// ------------------------------------------------------------------ k_ga
constexpr int kGaMaxAcc = 2;
constexpr size_t kGaWorkspaceBytes = (size_t)kGaMaxAcc * kDetMaxGrid * sizeof(double);

// <A[a], B[b]> as hgnn_edge_dot_f32 forms it.  VEC (D % 4 == 0, 16-byte aligned tables; k_edge_dot with 4 lanes per
// row): lane c holds q_c = the 4-term expression of its 16-byte column, the row is (q0 + q1) + (q2 + q3) with 0 for
// an absent column.  Otherwise (k_edge_dot_scalar): lane c holds A[c] B[c], summed by the xor tree over 64 lanes of
// which all but the first D hold 0, i.e. the balanced tree over 16 padded products.
template <bool VEC>
__device__ __forceinline__ float ga_dot(const float* __restrict__ pa, const float* __restrict__ pb, int D) {
    if (VEC) {
        float q[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float s = 0.f;
            if (c * 4 < D) {
                f32x4 x = *(const f32x4*)(pa + c * 4);
                f32x4 y = *(const f32x4*)(pb + c * 4);
                s += x.x * y.x + x.y * y.y + x.z * y.z + x.w * y.w;
            }
            q[c] = s;
        }
        return (q[0] + q[1]) + (q[2] + q[3]);
    }
    float p[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        float t = 0.f;
        if (c < D) t += pa[c] * pb[c];
        p[c] = t;
    }
#pragma unroll
    for (int off = 1; off < 16; off <<= 1)
#pragma unroll
        for (int c = 0; c < 16; c += 2 * off) p[c] += p[c + off];
    return p[0];
}

template <class IT, bool VEC, bool TRAIN>
__global__ __launch_bounds__(kBlock) void k_ga_dot(const float* __restrict__ A, int64_t Na,
                                                   const float* __restrict__ B, int64_t Nb, int D,
                                                   const IT* __restrict__ ga, const IT* __restrict__ gb, int64_t E,
                                                   float* __restrict__ x, double* __restrict__ partials) {
    __shared__ double lds[kWavesPerBlock];
    double acc[2] = {0.0, 0.0};
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < E; e += (int64_t)gridDim.x * kBlock) {
        const int64_t a = (int64_t)ga[e], b = (int64_t)gb[e];
        float v = 0.f;                                        // an id out of range: no address is formed from it
        if (a >= 0 && a < Na && b >= 0 && b < Nb) v = ga_dot<VEC>(A + a * D, B + b * D, D);
        x[e] = v;
        if (TRAIN) {
            acc[0] += (double)v;
            acc[1] += (double)v * (double)v;
        }
    }
    if (TRAIN) write_partials<2>(acc, lds, partials);
}

// one workgroup.  Training: mu, biased var from the partials, then nn.BatchNorm1d's running update (unbiased
// variance, momentum < 0 = cumulative average 1 / num_batches_tracked).  Eval: the running statistics.
__global__ __launch_bounds__(kBlock) void k_ga_stats(const double* __restrict__ partials, int n_partials, int64_t E,
                                                     int train, double eps, double momentum,
                                                     float* __restrict__ running_mean,
                                                     float* __restrict__ running_var,
                                                     int64_t* __restrict__ num_batches_tracked,
                                                     double* __restrict__ state) {
    __shared__ double lds[kWavesPerBlock];
    double tot[2] = {0.0, 0.0};
    if (train) total_partials<2>(partials, n_partials, lds, tot);
    if (threadIdx.x != 0) return;
    double mu, var;
    if (train) {
        const double n = (double)E;
        mu = tot[0] / n;
        var = tot[1] / n - mu * mu;
        if (var < 0.0) var = 0.0;
        double m = momentum;
        if (num_batches_tracked != nullptr) {
            const int64_t t = *num_batches_tracked + 1;
            *num_batches_tracked = t;
            if (m < 0.0) m = 1.0 / (double)t;
        }
        if (m < 0.0) m = 0.0;
        *running_mean = (float)((1.0 - m) * (double)*running_mean + m * mu);
        *running_var = (float)((1.0 - m) * (double)*running_var + m * (var * n / (n - 1.0)));
    } else {
        mu = (double)*running_mean;
        var = (double)*running_var;
    }
    state[HGNN_GA_MEAN] = mu;
    state[HGNN_GA_VAR] = var;
    state[HGNN_GA_RSTD] = 1.0 / sqrt(var + eps);
    state[HGNN_GA_E] = (double)E;
}

template <bool EXP>
__device__ __forceinline__ float ga_phi(float z) {
    return EXP ? expf(z) : 1.f / (1.f + expf(-z));
}

template <bool EXP>
__global__ __launch_bounds__(kBlock) void k_ga_apply(const float* __restrict__ x, int64_t E,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     const double* __restrict__ state, float* __restrict__ logits,
                                                     float* __restrict__ f, double* __restrict__ partials) {
    __shared__ double lds[kWavesPerBlock];
    const float mu = (float)state[HGNN_GA_MEAN], rstd = (float)state[HGNN_GA_RSTD], g = gamma[0], b = beta[0];
    double acc[1] = {0.0};
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < E; e += (int64_t)gridDim.x * kBlock) {
        const float z = g * ((x[e] - mu) * rstd) + b;
        const float v = ga_phi<EXP>(z);
        logits[e] = z;
        f[e] = v;
        acc[0] += (double)v;
    }
    write_partials<1>(acc, lds, partials);
}

// one workgroup: the partials of NACC sums -> state[slot .. slot + NACC)
template <int NACC>
__global__ __launch_bounds__(kBlock) void k_ga_finish(const double* __restrict__ partials, int n_partials, int slot,
                                                      double* __restrict__ state) {
    __shared__ double lds[kWavesPerBlock];
    double tot[NACC];
    total_partials<NACC>(partials, n_partials, lds, tot);
    if (threadIdx.x == 0)
        for (int k = 0; k < NACC; ++k) state[slot + k] = tot[k];
}

__global__ __launch_bounds__(kBlock) void k_ga_scale(float* __restrict__ w, int64_t E,
                                                     const double* __restrict__ state) {
    const float inv_m = (float)((double)E / state[HGNN_GA_SUMF]);
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < E; e += (int64_t)gridDim.x * kBlock)
        w[e] = w[e] * inv_m;
}

// backward, with norm: partial sums of g_w f (f recomputed from x with the forward's float32 operations)
template <bool EXP>
__global__ __launch_bounds__(kBlock) void k_ga_bwd_gf(const float* __restrict__ x, int64_t E,
                                                      const float* __restrict__ gamma,
                                                      const float* __restrict__ beta,
                                                      const double* __restrict__ state,
                                                      const float* __restrict__ g_w,
                                                      double* __restrict__ partials) {
    __shared__ double lds[kWavesPerBlock];
    const float mu = (float)state[HGNN_GA_MEAN], rstd = (float)state[HGNN_GA_RSTD], g = gamma[0], b = beta[0];
    double acc[1] = {0.0};
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < E; e += (int64_t)gridDim.x * kBlock) {
        const float v = ga_phi<EXP>(g * ((x[e] - mu) * rstd) + b);
        acc[0] += (double)g_w[e] * (double)v;
    }
    write_partials<1>(acc, lds, partials);
}

// G_e = g_f phi'(z) + g_logits -> G (float32), partial sums of G and G xhat
template <bool EXP, bool NORM>
__global__ __launch_bounds__(kBlock) void k_ga_bwd_G(const float* __restrict__ x, int64_t E,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     const double* __restrict__ state, const float* __restrict__ g_w,
                                                     const float* __restrict__ g_logits, float* __restrict__ G,
                                                     double* __restrict__ partials) {
    __shared__ double lds[kWavesPerBlock];
    const float mu = (float)state[HGNN_GA_MEAN], rstd = (float)state[HGNN_GA_RSTD], g = gamma[0], b = beta[0];
    float c1 = 1.f, c0 = 0.f;                                 // g_f = c1 g_w - c0
    if (NORM) {
        const double n = state[HGNN_GA_E], m = state[HGNN_GA_SUMF] / n;
        c1 = (float)(1.0 / m);
        c0 = (float)(state[HGNN_GA_SGF] / (n * m * m));
    }
    double acc[2] = {0.0, 0.0};
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < E; e += (int64_t)gridDim.x * kBlock) {
        const float xh = (x[e] - mu) * rstd;
        const float v = ga_phi<EXP>(g * xh + b);
        const float gf = NORM ? c1 * g_w[e] - c0 : g_w[e];
        float t = gf * (EXP ? v : v * (1.f - v));
        if (g_logits != nullptr) t += g_logits[e];
        G[e] = t;
        acc[0] += (double)t;
        acc[1] += (double)t * (double)xh;
    }
    write_partials<2>(acc, lds, partials);
}

// g_x = gamma rstd (G - dbeta / E - xhat dgamma / E) in training, gamma rstd G in eval; thread 0 writes (dgamma, dbeta)
__global__ __launch_bounds__(kBlock) void k_ga_bwd_x(const float* __restrict__ x, int64_t E,
                                                     const float* __restrict__ gamma,
                                                     const double* __restrict__ state, int train,
                                                     float* __restrict__ g_x, float* __restrict__ g_bn) {
    const float mu = (float)state[HGNN_GA_MEAN], rstd = (float)state[HGNN_GA_RSTD];
    const float k = gamma[0] * rstd;
    const double n = state[HGNN_GA_E];
    const float mb = train ? (float)(state[HGNN_GA_DBETA] / n) : 0.f;
    const float mg = train ? (float)(state[HGNN_GA_DGAMMA] / n) : 0.f;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        g_bn[0] = (float)state[HGNN_GA_DGAMMA];
        g_bn[1] = (float)state[HGNN_GA_DBETA];
    }
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < E; e += (int64_t)gridDim.x * kBlock) {
        const float xh = (x[e] - mu) * rstd;
        g_x[e] = k * (g_x[e] - mb - xh * mg);
    }
}

int ga_check_fn(const char* who, int32_t fn, int32_t flags) {
    HGNN_REQUIRE(fn == HGNN_GA_FN_SIGMOID || fn == HGNN_GA_FN_EXP, "%s: fn must be HGNN_GA_FN_SIGMOID or HGNN_GA_FN_EXP",
                 who);
    HGNN_REQUIRE((flags & ~(HGNN_GA_TRAINING | HGNN_GA_NORM)) == 0, "%s: unknown flag bits", who);
    return HGNN_OK;
}

}  // namespace
}  // namespace hgnn

using namespace hgnn;

extern "C" int hgnn_knn_edges_workspace_bytes(int64_t nq, int32_t K, int64_t n_pts, int32_t sym, size_t* bytes) {
    const char* who = "hgnn_knn_edges_workspace_bytes";
    HGNN_REQUIRE(bytes != nullptr, "%s: bytes is NULL", who);
    HGNN_REQUIRE(nq >= 0 && K >= 1 && n_pts >= 0, "%s: need nq >= 0, K >= 1, n_pts >= 0", who);
    HGNN_REQUIRE(nq <= kGcMaxSlots / K, "%s: nq * K must stay below 2^30", who);
    const int64_t n = nq > n_pts ? nq : n_pts;
    HGNN_REQUIRE(n <= ((int64_t)1 << 31), "%s: max(nq, n_pts) = %lld exceeds 2^31", who, (long long)n);
    GcWorkspace w;
    int rc = gc_layout(nq * K, sym != 0, gc_bits(n), &w, nullptr);
    if (rc != HGNN_OK) return rc;
    *bytes = w.total;
    return HGNN_OK;
}

extern "C" int hgnn_knn_edges(const int64_t* idx, int64_t nq, int32_t K, int64_t n_pts, int32_t sym, int64_t* edges,
                              int64_t cap, int64_t* count_and_status, void* workspace, size_t workspace_bytes,
                              hgnn_stream_t stream_) {
    const char* who = "hgnn_knn_edges";
    hipStream_t stream = (hipStream_t)stream_;
    HGNN_REQUIRE(nq >= 0 && K >= 1 && n_pts >= 0, "%s: need nq >= 0, K >= 1, n_pts >= 0", who);
    HGNN_REQUIRE(nq <= kGcMaxSlots / K, "%s: nq * K must stay below 2^30", who);
    const int64_t n = nq > n_pts ? nq : n_pts;
    HGNN_REQUIRE(n <= ((int64_t)1 << 31), "%s: max(nq, n_pts) = %lld exceeds 2^31", who, (long long)n);
    HGNN_REQUIRE(count_and_status != nullptr, "%s: count_and_status is NULL", who);
    const int64_t slots = nq * K;
    HGNN_REQUIRE(cap >= (sym ? 2 : 1) * slots, "%s: edges needs room for %lld pairs per row", who,
                 (long long)((sym ? 2 : 1) * slots));
    HGNN_REQUIRE(slots == 0 || (idx != nullptr && edges != nullptr), "%s: NULL pointer", who);
    const int bits = gc_bits(n);
    GcWorkspace w;
    int rc = gc_layout(slots, sym != 0, bits, &w, stream);
    if (rc != HGNN_OK) return rc;
    if (slots > 0 && (workspace == nullptr || workspace_bytes < w.total)) {
        set_error("%s: workspace too small (%zu < %zu)", who, workspace_bytes, w.total);
        return HGNN_ERR_WORKSPACE;
    }
    HGNN_CHECK_HIP(hipMemsetAsync(count_and_status, 0, 2 * sizeof(int64_t), stream));
    if (slots == 0) return HGNN_OK;
    char* ws = (char*)workspace;
    void* temp = ws + w.temp;
    size_t tb = w.temp_bytes;
    if (!sym) {
        int32_t* pos = (int32_t*)(ws + w.pos);
        HGNN_CHECK_HIP(rocprim::exclusive_scan(temp, tb, rocprim::make_transform_iterator(idx, GcValid{n_pts}), pos,
                                               (int32_t)0, (size_t)slots, rocprim::plus<int32_t>(), stream));
        k_gc_fill<<<gc_blocks(slots), kBlock, 0, stream>>>(idx, slots, K, n_pts, pos, cap, edges, count_and_status);
    } else {
        uint64_t *key = (uint64_t*)(ws + w.key), *key_s = (uint64_t*)(ws + w.key_s), *ukey = (uint64_t*)(ws + w.ukey);
        size_t* n_unique = (size_t*)(ws + w.count);
        k_gc_keys<<<gc_blocks(slots), kBlock, 0, stream>>>(idx, slots, K, n_pts, bits, key, count_and_status);
        HGNN_CHECK_HIP(rocprim::radix_sort_keys(temp, tb, key, key_s, (size_t)(2 * slots), 0u,
                                                (unsigned)(2 * bits + 1), stream));
        HGNN_CHECK_HIP(rocprim::unique(temp, tb, key_s, ukey, n_unique, (size_t)(2 * slots),
                                       rocprim::equal_to<uint64_t>(), stream));
        k_gc_decode<<<gc_blocks(2 * slots), kBlock, 0, stream>>>(ukey, n_unique, bits, cap, edges, count_and_status);
    }
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}

extern "C" int hgnn_graph_attention_workspace_bytes(int64_t E, int32_t backward, size_t* bytes) {
    HGNN_REQUIRE(bytes != nullptr, "hgnn_graph_attention_workspace_bytes: bytes is NULL");
    HGNN_REQUIRE(E >= 0, "hgnn_graph_attention_workspace_bytes: need E >= 0");
    (void)backward;
    *bytes = kGaWorkspaceBytes;
    return HGNN_OK;
}

extern "C" int hgnn_graph_attention_forward(const float* A, int64_t Na, const float* B, int64_t Nb, int32_t D,
                                            const void* graph, int32_t index_dtype, int64_t E, const float* bn_weight,
                                            const float* bn_bias, float* running_mean, float* running_var,
                                            int64_t* num_batches_tracked, double eps, double momentum, int32_t flags,
                                            int32_t fn, float* x, float* logits, float* weights, double* state,
                                            void* workspace, size_t workspace_bytes, hgnn_stream_t stream_) {
    const char* who = "hgnn_graph_attention_forward";
    hipStream_t stream = (hipStream_t)stream_;
    int rc = ga_check_fn(who, fn, flags);
    if (rc != HGNN_OK) return rc;
    const bool train = (flags & HGNN_GA_TRAINING) != 0, norm = (flags & HGNN_GA_NORM) != 0;
    HGNN_REQUIRE(E >= 0 && Na >= 0 && Nb >= 0, "%s: need E, Na, Nb >= 0", who);
    HGNN_REQUIRE(D >= 1 && D <= HGNN_GA_MAX_DIM, "%s: D = %d outside 1..%d", who, D, HGNN_GA_MAX_DIM);
    HGNN_REQUIRE(index_dtype == HGNN_DT_I32 || index_dtype == HGNN_DT_I64, "%s: index_dtype must be I32 or I64", who);
    HGNN_REQUIRE(!train || E >= 2, "%s: training mode needs more than 1 edge", who);
    if (E == 0) return HGNN_OK;
    HGNN_REQUIRE(A && B && graph && bn_weight && bn_bias && running_mean && running_var && x && logits && weights &&
                     state,
                 "%s: NULL pointer", who);
    HGNN_REQUIRE_WORKSPACE(who, workspace, workspace_bytes, kGaWorkspaceBytes);
    double* partials = (double*)workspace;
    const unsigned grid = det_grid(E);
    const bool vec = D % 4 == 0 && (uintptr_t)A % 16 == 0 && (uintptr_t)B % 16 == 0;
    auto dot = [&](auto it, auto vk, auto tr) {
        using IT = decltype(it);
        k_ga_dot<IT, decltype(vk)::value, decltype(tr)::value><<<grid, kBlock, 0, stream>>>(
            A, Na, B, Nb, D, (const IT*)graph, (const IT*)graph + E, E, x, partials);
    };
    auto with_train = [&](auto it, auto vk) {
        if (train) dot(it, vk, std::true_type{});
        else dot(it, vk, std::false_type{});
    };
    auto with_vec = [&](auto it) {
        if (vec) with_train(it, std::true_type{});
        else with_train(it, std::false_type{});
    };
    if (index_dtype == HGNN_DT_I64) with_vec((int64_t)0);
    else with_vec((int32_t)0);
    k_ga_stats<<<1, kBlock, 0, stream>>>(partials, (int)grid, E, train ? 1 : 0, eps, momentum, running_mean,
                                         running_var, num_batches_tracked, state);
    if (fn == HGNN_GA_FN_EXP) k_ga_apply<true><<<grid, kBlock, 0, stream>>>(x, E, bn_weight, bn_bias, state, logits,
                                                                            weights, partials);
    else k_ga_apply<false><<<grid, kBlock, 0, stream>>>(x, E, bn_weight, bn_bias, state, logits, weights, partials);
    k_ga_finish<1><<<1, kBlock, 0, stream>>>(partials, (int)grid, HGNN_GA_SUMF, state);
    if (norm) k_ga_scale<<<grid, kBlock, 0, stream>>>(weights, E, state);
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}

extern "C" int hgnn_graph_attention_backward(const float* x, int64_t E, const float* bn_weight, const float* bn_bias,
                                             int32_t flags, int32_t fn, double* state, const float* g_w,
                                             const float* g_logits, float* g_x, float* g_bn, void* workspace,
                                             size_t workspace_bytes, hgnn_stream_t stream_) {
    const char* who = "hgnn_graph_attention_backward";
    hipStream_t stream = (hipStream_t)stream_;
    int rc = ga_check_fn(who, fn, flags);
    if (rc != HGNN_OK) return rc;
    const bool train = (flags & HGNN_GA_TRAINING) != 0, norm = (flags & HGNN_GA_NORM) != 0;
    HGNN_REQUIRE(E >= 1, "%s: need E >= 1", who);
    HGNN_REQUIRE(x && bn_weight && bn_bias && state && g_w && g_x && g_bn, "%s: NULL pointer", who);
    HGNN_REQUIRE_WORKSPACE(who, workspace, workspace_bytes, kGaWorkspaceBytes);
    double* partials = (double*)workspace;
    const unsigned grid = det_grid(E);
    const bool ex = fn == HGNN_GA_FN_EXP;
    if (norm) {
        if (ex) k_ga_bwd_gf<true><<<grid, kBlock, 0, stream>>>(x, E, bn_weight, bn_bias, state, g_w, partials);
        else k_ga_bwd_gf<false><<<grid, kBlock, 0, stream>>>(x, E, bn_weight, bn_bias, state, g_w, partials);
        k_ga_finish<1><<<1, kBlock, 0, stream>>>(partials, (int)grid, HGNN_GA_SGF, state);
    }
    auto launch_G = [&](auto e_, auto n_) {
        k_ga_bwd_G<decltype(e_)::value, decltype(n_)::value><<<grid, kBlock, 0, stream>>>(
            x, E, bn_weight, bn_bias, state, g_w, g_logits, g_x, partials);
    };
    if (ex && norm) launch_G(std::true_type{}, std::true_type{});
    else if (ex) launch_G(std::true_type{}, std::false_type{});
    else if (norm) launch_G(std::false_type{}, std::true_type{});
    else launch_G(std::false_type{}, std::false_type{});
    k_ga_finish<2><<<1, kBlock, 0, stream>>>(partials, (int)grid, HGNN_GA_DBETA, state);
    k_ga_bwd_x<<<grid, kBlock, 0, stream>>>(x, E, bn_weight, state, train ? 1 : 0, g_x, g_bn);
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}
