// k_opt_*: the update of the four training bases as one operator: Trainer(gradient_clip_val) = clip_grad_norm_ and
// torch.optim.AdamW(betas, eps, amsgrad=True, weight_decay) (reference Modules/*/..._base.py configure_optimizers).
// For every parameter tensor with a gradient, in float32 and in torch's order:
//
//   total_norm = sqrt(sum over ALL tensors of g^2)        coef = min(1, max_norm / (total_norm + 1e-6))   (float32)
//   g' = g coef    p *= 1 - lr wd    m += (g' - m)(1 - b1)    v = v b2 + (1 - b2) g' g'    vmax = max(vmax, v)
//   denom = sqrt(vmax) / sqrt(bc2) + eps    p -= (lr / bc1) m / denom            bc1 = 1 - b1^t, bc2 = 1 - b2^t
//
// The tensors are described by a TABLE (hgnn_opt_entry, one per tensor): p, g, the element offset of the tensor's m, v
// and vmax in three flat state buffers, numel, the index of its first CHUNK and the scalars of this step, which the
// host computes in double.  A chunk is HGNN_OPT_CHUNK consecutive elements of ONE tensor; chunk c belongs to the last
// entry whose first_chunk <= c.  The map depends on the tensor sizes alone.  Inside a chunk, thread t owns the
// elements 4 (t + 256 j) .. + 3 for j = 0 .. 3, whether they are loaded as one 16-byte word or one by one.
//
// k_opt_sumsq: sum of g^2 in float64 -- per thread in that fixed order, per workgroup through the fixed tree
// (det_reduce.h's block_sum) -- one partial per workgroup; k_opt_norm_finish adds the partials in index order and
// writes state = {total_norm, coef, sum}.  The grid is a function of the chunk count alone, so the bits are too.
// k_opt_adamw: ONE pass, every array read once and written once.  No atomics other than the status atomicOr.
#include "common.h"
#include "det_reduce.h"
#include <cmath>
#include <type_traits>

// every float32 operation of this file is rounded on its own: no contraction into fused multiply-adds, so the 16-byte
// and the element-wise path give the same bits and the order of the update is the one written down above
#pragma clang fp contract(off)

namespace hgnn {
namespace {

constexpr int kOptChunk = HGNN_OPT_CHUNK;
constexpr int kOptGroups = kOptChunk / (4 * kBlock);    // 16-byte groups per thread and chunk
static_assert(kOptGroups * 4 * kBlock == kOptChunk, "a chunk is a whole number of 16-byte groups per thread");

enum { kGradsKeep = 0, kGradsZero = 1, kGradsWrite = 2 };

// the entry of chunk c: the last one whose first_chunk <= c (empty tensors, which own no chunk, sort before it)
__device__ __forceinline__ int opt_find(const hgnn_opt_entry* __restrict__ table, int n_tensors, int64_t c) {
    int lo = 0, hi = n_tensors - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].first_chunk <= c) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// p and g come out of the table, so the compiler cannot know that they point to global memory: say so, or every
// access becomes a flat one that waits on both counters
typedef __attribute__((address_space(1))) float gf32;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) f32x4 gf32x4;

__device__ __forceinline__ gf32* opt_global(const float* q) { return (gf32*)q; }

__device__ __forceinline__ bool opt_aligned16(const void* a, const void* b) {
    return (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
}

__device__ __forceinline__ void opt_sumsq4(double& acc, f32x4 t) {
#pragma unroll
    for (int k = 0; k < 4; ++k) acc += (double)t[k] * (double)t[k];
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_opt_sumsq(const hgnn_opt_entry* __restrict__ table, int n_tensors,
                                                      int64_t n_chunks, double* __restrict__ partials) {
    __shared__ double lds[kWavesPerBlock];
    double acc = 0.0;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const hgnn_opt_entry e = table[opt_find(table, n_tensors, c)];
        const int64_t first = (c - e.first_chunk) * kOptChunk;
        const int64_t left = e.numel - first;
        const int n = (int)(left < kOptChunk ? left : kOptChunk);
        const gf32* g = opt_global(e.g + first);
        const bool vec = VEC && opt_aligned16(e.g, e.g);
        if (vec && n == kOptChunk) {                                   // a whole chunk: all loads in flight at once
            f32x4 t[kOptGroups];
#pragma unroll
            for (int j = 0; j < kOptGroups; ++j) t[j] = ((const gf32x4*)g)[threadIdx.x + j * kBlock];
#pragma unroll
            for (int j = 0; j < kOptGroups; ++j) opt_sumsq4(acc, t[j]);
        } else {
            for (int j = 0; j < kOptGroups; ++j) {
                const int i0 = 4 * ((int)threadIdx.x + j * kBlock);
                if (i0 >= n) break;
                if (vec && i0 + 4 <= n) {
                    opt_sumsq4(acc, ((const gf32x4*)g)[i0 / 4]);
                } else {
                    for (int i = i0; i < i0 + 4 && i < n; ++i) {
                        const double x = (double)g[i];
                        acc += x * x;
                    }
                }
            }
        }
    }
    const double s = block_sum(acc, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;          // det_reduce.h write_partials, one accumulator
}

// one workgroup: thread t adds partials t, t + 256, .. in that order, then the fixed tree.  coef in float32 as
// clip_grad_norm_ forms it: max_norm / (total_norm + 1e-6), clamp(max = 1); a NaN norm gives a NaN coefficient.
__global__ __launch_bounds__(kBlock) void k_opt_norm_finish(const double* __restrict__ partials, int n_partials,
                                                            float max_norm, double* __restrict__ state,
                                                            int32_t* __restrict__ status) {
    __shared__ double lds[kWavesPerBlock];
    double v = 0.0;
    for (int j = threadIdx.x; j < n_partials; j += kBlock) v += partials[j];
    const double sum = block_sum(v, lds);
    if (threadIdx.x == 0) {
        const double norm = sqrt(sum);
        const float c = max_norm / ((float)norm + 1e-6f);
        state[HGNN_OPT_NORM] = norm;
        state[HGNN_OPT_COEF] = (double)(c > 1.f ? 1.f : c);         // NaN > 1 is false: NaN stays
        state[HGNN_OPT_SUMSQ] = sum;
        if (!(fabs(norm) <= 1.79769313486231570e308)) atomicOr(status, HGNN_OPT_ST_NONFINITE);   // inf or NaN
    }
}

// one element; g is already clipped
template <bool AMSGRAD>
__device__ __forceinline__ void opt_update(float& p, float g, float& m, float& v, float& vmax,
                                           const hgnn_opt_entry& e) {
    p = p * e.decay;
    m = m + (g - m) * e.one_minus_b1;
    v = v * e.b2 + (e.one_minus_b2 * g) * g;
    float top = v;
    if (AMSGRAD) {
        vmax = (v > vmax || v != v) ? v : vmax;                      // torch.maximum keeps NaN
        top = vmax;
    }
    const float denom = sqrtf(top) * e.inv_sqrt_bc2 + e.eps;
    p = p - e.step_size * (m / denom);
}

template <bool AMSGRAD, bool CLIP>
__device__ __forceinline__ void opt_update4(f32x4& p, f32x4& g, f32x4& m, f32x4& v, f32x4& x, float coef,
                                            const hgnn_opt_entry& e) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float pk = p[k], gk = CLIP ? g[k] * coef : g[k], mk = m[k], vk = v[k], xk = AMSGRAD ? x[k] : 0.f;
        opt_update<AMSGRAD>(pk, gk, mk, vk, xk, e);
        p[k] = pk, g[k] = gk, m[k] = mk, v[k] = vk, x[k] = xk;
    }
}

template <bool AMSGRAD, bool CLIP, int GRADS, bool VEC>
__global__ __launch_bounds__(kBlock) void k_opt_adamw(const hgnn_opt_entry* __restrict__ table, int n_tensors,
                                                      int64_t n_chunks, float* __restrict__ m_all,
                                                      float* __restrict__ v_all, float* __restrict__ vmax_all,
                                                      const double* __restrict__ state) {
    const float coef = CLIP ? (float)state[HGNN_OPT_COEF] : 1.f;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const hgnn_opt_entry e = table[opt_find(table, n_tensors, c)];
        const int64_t first = (c - e.first_chunk) * kOptChunk;
        const int64_t left = e.numel - first;
        const int n = (int)(left < kOptChunk ? left : kOptChunk);
        gf32* p = opt_global(e.p + first);
        gf32* g = opt_global(e.g + first);
        gf32* m = opt_global(m_all + e.offset + first);
        gf32* v = opt_global(v_all + e.offset + first);
        gf32* vm = AMSGRAD ? opt_global(vmax_all + e.offset + first) : nullptr;
        // m, v and vmax share one offset and the buffers' bases are 16-byte aligned (checked by the host); a chunk
        // starts a multiple of 16 bytes after its tensor
        const bool vec = VEC && opt_aligned16(e.p, e.g) && (e.offset & 3) == 0;
        if (vec && n == kOptChunk) {                                   // a whole chunk: all loads in flight at once
            f32x4 tp[kOptGroups], tg[kOptGroups], tm[kOptGroups], tv[kOptGroups], tx[kOptGroups];
#pragma unroll
            for (int j = 0; j < kOptGroups; ++j) {
                const int i = threadIdx.x + j * kBlock;
                tp[j] = ((const gf32x4*)p)[i];
                tg[j] = ((const gf32x4*)g)[i];
                tm[j] = ((const gf32x4*)m)[i];
                tv[j] = ((const gf32x4*)v)[i];
                tx[j] = AMSGRAD ? ((const gf32x4*)vm)[i] : zero4;
            }
#pragma unroll
            for (int j = 0; j < kOptGroups; ++j) {
                const int i = threadIdx.x + j * kBlock;
                opt_update4<AMSGRAD, CLIP>(tp[j], tg[j], tm[j], tv[j], tx[j], coef, e);
                ((gf32x4*)p)[i] = tp[j];
                ((gf32x4*)m)[i] = tm[j];
                ((gf32x4*)v)[i] = tv[j];
                if (AMSGRAD) ((gf32x4*)vm)[i] = tx[j];
                if (GRADS == kGradsZero) ((gf32x4*)g)[i] = zero4;
                if (GRADS == kGradsWrite && CLIP) ((gf32x4*)g)[i] = tg[j];
            }
        } else {
            for (int j = 0; j < kOptGroups; ++j) {
                const int i0 = 4 * ((int)threadIdx.x + j * kBlock);
                if (i0 >= n) break;
                if (vec && i0 + 4 <= n) {
                    const int i = i0 / 4;
                    f32x4 tp = ((const gf32x4*)p)[i], tg = ((const gf32x4*)g)[i], tm = ((const gf32x4*)m)[i],
                          tv = ((const gf32x4*)v)[i], tx = AMSGRAD ? ((const gf32x4*)vm)[i] : zero4;
                    opt_update4<AMSGRAD, CLIP>(tp, tg, tm, tv, tx, coef, e);
                    ((gf32x4*)p)[i] = tp;
                    ((gf32x4*)m)[i] = tm;
                    ((gf32x4*)v)[i] = tv;
                    if (AMSGRAD) ((gf32x4*)vm)[i] = tx;
                    if (GRADS == kGradsZero) ((gf32x4*)g)[i] = zero4;
                    if (GRADS == kGradsWrite && CLIP) ((gf32x4*)g)[i] = tg;
                } else {
                    for (int i = i0; i < i0 + 4 && i < n; ++i) {
                        float gi = g[i];
                        if (CLIP) gi = gi * coef;
                        float pi = p[i], mi = m[i], vi = v[i], xi = AMSGRAD ? vm[i] : 0.f;
                        opt_update<AMSGRAD>(pi, gi, mi, vi, xi, e);
                        p[i] = pi;
                        m[i] = mi;
                        v[i] = vi;
                        if (AMSGRAD) vm[i] = xi;
                        if (GRADS == kGradsZero) g[i] = 0.f;
                        if (GRADS == kGradsWrite && CLIP) g[i] = gi;
                    }
                }
            }
        }
    }
}

// one workgroup per chunk up to the cap, then a stride over the chunks; 0 chunks launch nothing
unsigned opt_grid(int64_t n_chunks) { return (unsigned)(n_chunks > kDetMaxGrid ? kDetMaxGrid : n_chunks); }

constexpr size_t kOptWorkspaceBytes = (size_t)kDetMaxGrid * sizeof(double);   // the partials

// the HOST copy of the table is what is checked: every kernel access lies inside [p, p + numel), [g, g + numel) and
// [offset, offset + numel) of the state buffers when it passes
int opt_check(const char* what, const hgnn_opt_entry* host_table, const hgnn_opt_entry* table, int64_t n_tensors,
              int64_t n_chunks, int64_t state_numel) {
    HGNN_REQUIRE(n_tensors >= 0 && n_tensors <= INT32_MAX && n_chunks >= 0 && state_numel >= 0,
                 "%s: need 0 <= n_tensors < 2^31, n_chunks >= 0, state_numel >= 0", what);
    HGNN_REQUIRE(n_tensors == 0 || (host_table != nullptr && table != nullptr), "%s: a table pointer is NULL", what);
    int64_t chunks = 0;
    for (int64_t i = 0; i < n_tensors; ++i) {
        const hgnn_opt_entry& e = host_table[i];
        HGNN_REQUIRE(e.numel >= 0 && e.offset >= 0 && e.offset <= state_numel && e.numel <= state_numel - e.offset,
                     "%s: entry %lld: [offset, offset + numel) = [%lld, + %lld) is outside the state buffers (%lld)",
                     what, (long long)i, (long long)e.offset, (long long)e.numel, (long long)state_numel);
        HGNN_REQUIRE(e.numel == 0 || (e.p != nullptr && e.g != nullptr), "%s: entry %lld: p or g is NULL", what,
                     (long long)i);
        HGNN_REQUIRE(((uintptr_t)e.p | (uintptr_t)e.g) % sizeof(float) == 0,
                     "%s: entry %lld: p or g is not 4-byte aligned", what, (long long)i);
        HGNN_REQUIRE(e.first_chunk == chunks, "%s: entry %lld: first_chunk is %lld, the sizes before it give %lld",
                     what, (long long)i, (long long)e.first_chunk, (long long)chunks);
        chunks += ceil_div(e.numel, kOptChunk);
    }
    HGNN_REQUIRE(chunks == n_chunks, "%s: n_chunks is %lld, the table's sizes give %lld", what, (long long)n_chunks,
                 (long long)chunks);
    return HGNN_OK;
}

}  // namespace
}  // namespace hgnn

using namespace hgnn;

extern "C" int hgnn_sizeof_opt_entry(void) { return (int)sizeof(hgnn_opt_entry); }

extern "C" int hgnn_optim_workspace_bytes(int64_t n_chunks, size_t* bytes) {
    HGNN_REQUIRE(bytes != nullptr, "hgnn_optim_workspace_bytes: bytes is NULL");
    HGNN_REQUIRE(n_chunks >= 0, "hgnn_optim_workspace_bytes: need n_chunks >= 0");
    *bytes = kOptWorkspaceBytes;
    return HGNN_OK;
}

extern "C" int hgnn_optim_grad_norm(const hgnn_opt_entry* host_table, const hgnn_opt_entry* table, int64_t n_tensors,
                                    int64_t n_chunks, double max_norm, int32_t flags, double* state, int32_t* status,
                                    void* workspace, size_t workspace_bytes, hgnn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = opt_check("hgnn_optim_grad_norm", host_table, table, n_tensors, n_chunks, INT64_MAX);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE(state != nullptr && status != nullptr, "hgnn_optim_grad_norm: NULL pointer");
    HGNN_REQUIRE((flags & ~HGNN_OPT_SCALAR) == 0, "hgnn_optim_grad_norm: only HGNN_OPT_SCALAR may be set in flags");
    HGNN_REQUIRE_WORKSPACE("hgnn_optim_grad_norm", workspace, workspace_bytes, kOptWorkspaceBytes);
    double* partials = (double*)workspace;
    const unsigned grid = opt_grid(n_chunks);
    if (grid > 0) {
        if (flags & HGNN_OPT_SCALAR)
            k_opt_sumsq<false><<<grid, kBlock, 0, stream>>>(table, (int)n_tensors, n_chunks, partials);
        else
            k_opt_sumsq<true><<<grid, kBlock, 0, stream>>>(table, (int)n_tensors, n_chunks, partials);
    }
    k_opt_norm_finish<<<1, kBlock, 0, stream>>>(partials, (int)grid, (float)max_norm, state, status);
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}

extern "C" int hgnn_optim_adamw_step(const hgnn_opt_entry* host_table, const hgnn_opt_entry* table, int64_t n_tensors,
                                     int64_t n_chunks, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq,
                                     int64_t state_numel, int32_t flags, const double* state, hgnn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = opt_check("hgnn_optim_adamw_step", host_table, table, n_tensors, n_chunks, state_numel);
    if (rc != HGNN_OK) return rc;
    constexpr int32_t known = HGNN_OPT_AMSGRAD | HGNN_OPT_CLIP | HGNN_OPT_ZERO_GRADS | HGNN_OPT_WRITE_GRADS |
                              HGNN_OPT_SCALAR;
    HGNN_REQUIRE((flags & ~known) == 0, "hgnn_optim_adamw_step: unknown bit in flags");
    HGNN_REQUIRE(!((flags & HGNN_OPT_ZERO_GRADS) && (flags & HGNN_OPT_WRITE_GRADS)),
                 "hgnn_optim_adamw_step: HGNN_OPT_ZERO_GRADS and HGNN_OPT_WRITE_GRADS exclude each other");
    HGNN_REQUIRE(!(flags & HGNN_OPT_CLIP) || state != nullptr,
                 "hgnn_optim_adamw_step: HGNN_OPT_CLIP needs the state hgnn_optim_grad_norm wrote");
    if (n_chunks == 0) return HGNN_OK;
    HGNN_REQUIRE(exp_avg != nullptr && exp_avg_sq != nullptr &&
                     (!(flags & HGNN_OPT_AMSGRAD) || max_exp_avg_sq != nullptr),
                 "hgnn_optim_adamw_step: a state buffer is NULL");
    HGNN_REQUIRE(((uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)max_exp_avg_sq) % 16 == 0,
                 "hgnn_optim_adamw_step: the state buffers must be 16-byte aligned");
    const unsigned grid = opt_grid(n_chunks);
    auto launch = [&](auto ams, auto clip, auto grads, auto vec) {
        k_opt_adamw<decltype(ams)::value, decltype(clip)::value, decltype(grads)::value, decltype(vec)::value>
            <<<grid, kBlock, 0, stream>>>(table, (int)n_tensors, n_chunks, exp_avg, exp_avg_sq, max_exp_avg_sq, state);
    };
    auto with_vec = [&](auto ams, auto clip, auto grads) {
        if (flags & HGNN_OPT_SCALAR) launch(ams, clip, grads, std::false_type{});
        else launch(ams, clip, grads, std::true_type{});
    };
    auto with_grads = [&](auto ams, auto clip) {
        if (flags & HGNN_OPT_ZERO_GRADS) with_vec(ams, clip, std::integral_constant<int, kGradsZero>{});
        else if (flags & HGNN_OPT_WRITE_GRADS) with_vec(ams, clip, std::integral_constant<int, kGradsWrite>{});
        else with_vec(ams, clip, std::integral_constant<int, kGradsKeep>{});
    };
    auto with_clip = [&](auto ams) {
        if (flags & HGNN_OPT_CLIP) with_grads(ams, std::true_type{});
        else with_grads(ams, std::false_type{});
    };
    if (flags & HGNN_OPT_AMSGRAD) with_clip(std::true_type{});
    else with_clip(std::false_type{});
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}
