// Segmented min / max with arg output, and exact integer sums, on the destination plan (gfx950, wave64):
//
//   k_seg_arg        : torch_scatter.scatter_min / scatter_max (reference BipartiteClassification/
//                      bipartite_classification_base.py:158, gMRT/gmrt_base.py:165, tracking_utils.py:41)
//                      and the integer scatter_sum of tracking_utils.py:37 (op SUM, int32 / int64 only)
//   k_seg_arg_narrow : the same for rows that are not a whole number of 4-element columns (F = 1: the BC loss)
//   k_arg_combine    : second pass over the partial results of split destinations
//   k_arg_scatter    : backward of min / max, grad_src[arg[d,f], f] = grad_out[d,f]
//
// The plan's work list is walked exactly as k_seg_reduce walks it (segreduce.hip): one wave per work
// item, RL lanes x one 4-element column per row, U rows in flight.  Min / max reduce (value, position)
// pairs and combine them lexicographically -- the better value first, then the smaller position -- so
// ties go to the first occurrence along `dim` and the result does not depend on how the plan chunks a
// long list, nor on which lane saw which row.  A NaN is never a candidate (strict comparisons), so a
// list of NaN only is empty: out = 0, arg = M.  No atomics: every out / arg element is written once,
// split destinations through int32 partial positions and a second pass.
#include "rows_common.h"
#include <climits>

namespace hgnn {
namespace sarg {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef long long i64x2 __attribute__((ext_vector_type(2)));

constexpr int32_t kNone = INT32_MAX;  // "no candidate": loses to every real position

template <int DT> struct Ty;
template <> struct Ty<HGNN_DT_F32> { typedef float T; typedef float K; };
template <> struct Ty<HGNN_DT_BF16> { typedef uint16_t T; typedef float K; };   // bf16 widens to fp32 exactly
template <> struct Ty<HGNN_DT_I32> { typedef int32_t T; typedef int K; };
template <> struct Ty<HGNN_DT_I64> { typedef int64_t T; typedef long long K; };

template <int DT>
__device__ __forceinline__ typename Ty<DT>::K ld1(const void* base, size_t off) {
    if constexpr (DT == HGNN_DT_BF16)
        return __builtin_bit_cast(float, (unsigned)((const uint16_t*)base)[off] << 16);
    else
        return ((const typename Ty<DT>::T*)base)[off];
}

template <int DT>
__device__ __forceinline__ void st1(void* base, size_t off, typename Ty<DT>::K x) {
    if constexpr (DT == HGNN_DT_BF16)
        ((uint16_t*)base)[off] = (uint16_t)(__builtin_bit_cast(unsigned, x) >> 16);
    else
        ((typename Ty<DT>::T*)base)[off] = x;
}

// 4 consecutive elements at element offset `off` (a multiple of 4): one 16-B load (8 B for bf16, 2 x 16 B for int64)
template <int DT>
__device__ __forceinline__ void ld4(const void* base, size_t off, typename Ty<DT>::K (&x)[4]) {
    if constexpr (DT == HGNN_DT_F32) {
        const f32x4 v = __builtin_nontemporal_load((const f32x4*)((const float*)base + off));
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else if constexpr (DT == HGNN_DT_I32) {
        const i32x4 v = __builtin_nontemporal_load((const i32x4*)((const int32_t*)base + off));
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else if constexpr (DT == HGNN_DT_BF16) {
        const u32x2 v = __builtin_nontemporal_load((const u32x2*)((const uint16_t*)base + off));
        x[0] = __builtin_bit_cast(float, v.x << 16);
        x[1] = __builtin_bit_cast(float, v.x & 0xffff0000u);
        x[2] = __builtin_bit_cast(float, v.y << 16);
        x[3] = __builtin_bit_cast(float, v.y & 0xffff0000u);
    } else {
        const i64x2* p = (const i64x2*)((const int64_t*)base + off);
        const i64x2 a = __builtin_nontemporal_load(p), b = __builtin_nontemporal_load(p + 1);
        x[0] = a.x; x[1] = a.y; x[2] = b.x; x[3] = b.y;
    }
}

template <int DT>
__device__ __forceinline__ void st4(void* base, size_t off, const typename Ty<DT>::K (&x)[4]) {
    if constexpr (DT == HGNN_DT_F32) {
        *(f32x4*)((float*)base + off) = f32x4{x[0], x[1], x[2], x[3]};
    } else if constexpr (DT == HGNN_DT_I32) {
        *(i32x4*)((int32_t*)base + off) = i32x4{x[0], x[1], x[2], x[3]};
    } else if constexpr (DT == HGNN_DT_BF16) {
        const unsigned b0 = __builtin_bit_cast(unsigned, x[0]) >> 16, b1 = __builtin_bit_cast(unsigned, x[1]) >> 16;
        const unsigned b2 = __builtin_bit_cast(unsigned, x[2]) >> 16, b3 = __builtin_bit_cast(unsigned, x[3]) >> 16;
        *(u32x2*)((uint16_t*)base + off) = u32x2{b0 | (b1 << 16), b2 | (b3 << 16)};
    } else {
        i64x2* p = (i64x2*)((int64_t*)base + off);
        p[0] = i64x2{x[0], x[1]};
        p[1] = i64x2{x[2], x[3]};
    }
}

__device__ __forceinline__ void st4_arg(int64_t* arg, size_t off, const int32_t (&p)[4], int64_t M) {
    i64x2* q = (i64x2*)(arg + off);
    q[0] = i64x2{p[0] == kNone ? M : (long long)p[0], p[1] == kNone ? M : (long long)p[1]};
    q[1] = i64x2{p[2] == kNone ? M : (long long)p[2], p[3] == kNone ? M : (long long)p[3]};
}

template <class K>
__device__ __forceinline__ bool is_nan(K x) {
    if constexpr (std::is_same<K, float>::value) return x != x;
    else return false;
}

template <class K>
__device__ __forceinline__ K add(K a, K b) {  // wrapping integer add (what torch's int sum does on overflow)
    typedef typename std::conditional<sizeof(K) == 8, unsigned long long, unsigned>::type U;
    return (K)((U)a + (U)b);
}

// fold candidate (x, px) into the running (y, py).  MIN / MAX: lexicographic on (value, position) with kNone
// losing to everything; SUM: plain integer add.
template <int OP, class K>
__device__ __forceinline__ void fold(K& y, int32_t& py, K x, int32_t px) {
    if constexpr (OP == HGNN_RED_SUM) {
        y = add(y, x);
    } else {
        const bool better = OP == HGNN_RED_MIN ? x < y : x > y;
        const bool take = px != kNone && (py == kNone || better || (x == y && px < py));
        y = take ? x : y;
        py = take ? px : py;
    }
}

template <int OP, class K>
__device__ __forceinline__ void fold_xor(K& y, int32_t& py, int off) {
    const K x = __shfl_xor(y, off);
    const int32_t px = OP == HGNN_RED_SUM ? 0 : __shfl_xor(py, off);
    fold<OP>(y, py, x, px);
}

// Wide rows (F % 4 == 0, 4 <= F <= 1024): RL lanes cover a row, one 4-element column each (VPL columns per
// lane beyond 256 elements); G = 64/RL rows per load instruction, U of them issued before the first fold.
template <int DT, int OP, int RL, int VPL, int U, int WPB>
__global__ __launch_bounds__(WPB * 64) void k_seg_arg(
    const void* __restrict__ src, int F, int nvec, const int32_t* __restrict__ perm,
    const int32_t* __restrict__ wi_begin, const int32_t* __restrict__ wi_end, const int32_t* __restrict__ wi_target,
    const int32_t* __restrict__ n_items_ptr, int64_t max_items, int64_t M, void* __restrict__ out,
    int64_t* __restrict__ arg, void* __restrict__ partial, int32_t* __restrict__ partial_arg) {
    typedef typename Ty<DT>::K K;
    constexpr int G = 64 / RL;
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
    const int n_items = *n_items_ptr;
    if (item >= n_items || item >= max_items) return;
    const int begin = __builtin_amdgcn_readfirstlane(wi_begin[item]);
    const int end = __builtin_amdgcn_readfirstlane(wi_end[item]);
    const int target = __builtin_amdgcn_readfirstlane(wi_target[item]);
    const int g = lane / RL;
    const int c = lane % RL;

    K best[VPL][4];
    int32_t bpos[VPL][4];
#pragma unroll
    for (int v = 0; v < VPL; ++v)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            best[v][k] = (K)0;
            bpos[v][k] = kNone;
        }

    for (int base = begin; base < end; base += 64) {
        const int n = (end - base) < 64 ? (end - base) : 64;
        int my_pos = 0;
        if (lane < n) my_pos = perm != nullptr ? perm[base + lane] : base + lane;
        for (int j = 0; j < n; j += G * U) {
            K val[U][VPL][4];
            int32_t pos[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int e = j + u * G + g;
                const int r = G == 1 ? __builtin_amdgcn_readlane(my_pos, (j + u) & 63) : __shfl(my_pos, e & 63);
                const bool ok = e < n;
                pos[u] = ok ? r : kNone;
                const size_t row = (size_t)(ok ? r : 0) * (size_t)F;
#pragma unroll
                for (int v = 0; v < VPL; ++v) {
                    const int cv = c + v * 64;
                    if (ok && cv < nvec) {
                        ld4<DT>(src, row + (size_t)cv * 4, val[u][v]);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k) val[u][v][k] = (K)0;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int v = 0; v < VPL; ++v)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const K x = val[u][v][k];
                        fold<OP>(best[v][k], bpos[v][k], x, is_nan(x) ? kNone : pos[u]);
                    }
        }
    }
    if (G > 1) {
#pragma unroll
        for (int off = RL; off < 64; off <<= 1)
#pragma unroll
            for (int v = 0; v < VPL; ++v)
#pragma unroll
                for (int k = 0; k < 4; ++k) fold_xor<OP>(best[v][k], bpos[v][k], off);
    }
    if (g == 0) {
#pragma unroll
        for (int v = 0; v < VPL; ++v) {
            const int cv = c + v * 64;
            if (cv >= nvec) continue;
            if (target >= 0) {
                const size_t o = (size_t)target * (size_t)F + (size_t)cv * 4;
                if (OP != HGNN_RED_SUM) {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (bpos[v][k] == kNone) best[v][k] = (K)0;
                    st4_arg(arg, o, bpos[v], M);
                }
                st4<DT>(out, o, best[v]);
            } else {
                const size_t o = (size_t)(~target) * (size_t)F + (size_t)cv * 4;
                st4<DT>(partial, o, best[v]);
                if (OP != HGNN_RED_SUM) *(i32x4*)(partial_arg + o) = i32x4{bpos[v][0], bpos[v][1], bpos[v][2], bpos[v][3]};
            }
        }
    }
}

// Any F (F = 1 is the BC loss, scatter_min(pt, pid)): the 64 lanes take 64 consecutive rows of the list, each
// column is folded per lane and then across the wave by an xor-shuffle tree.
template <int DT, int OP>
__global__ __launch_bounds__(256) void k_seg_arg_narrow(
    const void* __restrict__ src, int F, const int32_t* __restrict__ perm, const int32_t* __restrict__ wi_begin,
    const int32_t* __restrict__ wi_end, const int32_t* __restrict__ wi_target, const int32_t* __restrict__ n_items_ptr,
    int64_t max_items, int64_t M, void* __restrict__ out, int64_t* __restrict__ arg, void* __restrict__ partial,
    int32_t* __restrict__ partial_arg) {
    typedef typename Ty<DT>::K K;
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int n_items = *n_items_ptr;
    if (item >= n_items || item >= max_items) return;
    const int begin = __builtin_amdgcn_readfirstlane(wi_begin[item]);
    const int end = __builtin_amdgcn_readfirstlane(wi_end[item]);
    const int target = __builtin_amdgcn_readfirstlane(wi_target[item]);
    // the first 64 positions stay in a register across the columns (most lists are shorter)
    const int p0 = begin + lane;
    const int pos0 = p0 < end ? (perm != nullptr ? perm[p0] : p0) : kNone;
    for (int col = 0; col < F; ++col) {
        K y = (K)0;
        int32_t py = kNone;
        for (int base = begin; base < end; base += 64) {
            const int p = base + lane;
            int32_t pos = base == begin ? pos0 : (p < end ? (perm != nullptr ? perm[p] : p) : kNone);
            if (pos != kNone) {
                const K x = ld1<DT>(src, (size_t)pos * (size_t)F + col);
                fold<OP>(y, py, x, is_nan(x) ? kNone : pos);
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) fold_xor<OP>(y, py, off);
        if (lane == 0) {
            if (target >= 0) {
                const size_t o = (size_t)target * (size_t)F + col;
                if (OP != HGNN_RED_SUM) arg[o] = py == kNone ? M : (int64_t)py;
                st1<DT>(out, o, (OP != HGNN_RED_SUM && py == kNone) ? (K)0 : y);
            } else {
                const size_t o = (size_t)(~target) * (size_t)F + col;
                st1<DT>(partial, o, y);
                if (OP != HGNN_RED_SUM) partial_arg[o] = py;
            }
        }
    }
}

// split destinations: fold their partial rows in chunk order (lanes over columns)
template <int DT, int OP>
__global__ __launch_bounds__(256) void k_arg_combine(
    const void* __restrict__ partial, const int32_t* __restrict__ partial_arg, int F,
    const int32_t* __restrict__ split_dst, const int32_t* __restrict__ split_pbegin,
    const int32_t* __restrict__ n_split_ptr, int64_t max_split, int64_t M, void* __restrict__ out,
    int64_t* __restrict__ arg) {
    typedef typename Ty<DT>::K K;
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int n_split = *n_split_ptr;
    if (item >= n_split || item >= max_split) return;
    const int d = split_dst[item];
    const int qb = split_pbegin[item], qe = split_pbegin[item + 1];
    for (int col = lane; col < F; col += 64) {
        K y = (K)0;
        int32_t py = kNone;
        for (int q = qb; q < qe; ++q) {
            const size_t o = (size_t)q * (size_t)F + col;
            fold<OP>(y, py, ld1<DT>(partial, o), OP == HGNN_RED_SUM ? 0 : partial_arg[o]);
        }
        const size_t o = (size_t)d * (size_t)F + col;
        if (OP != HGNN_RED_SUM) arg[o] = py == kNone ? M : (int64_t)py;
        st1<DT>(out, o, (OP != HGNN_RED_SUM && py == kNone) ? (K)0 : y);
    }
}

template <class T>
__global__ __launch_bounds__(256) void k_arg_scatter(const int64_t* __restrict__ arg, const T* __restrict__ grad_out,
                                                     int64_t total, int F, int64_t M, T* __restrict__ grad_src) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t a = arg[i];
        if (a >= 0 && a < M) grad_src[a * F + i % F] = grad_out[i];
    }
}

// ------------------------------------------------------------------ dispatch
struct ArgArgs {
    const void* src;
    int F;
    int64_t M;  // rows of src: the arg of an empty list
    void* out;
    int64_t* arg;
    void* partial;
    int32_t* partial_arg;
    ItemView work, split;
};

// by row shape: rows in flight per wave (UH at a 1-KiB-wide fp32 row, K1's headline tile), waves per workgroup
constexpr int arg_rows_in_flight(int RL, int VPL, int UH) { return RL < 64 ? 4 : VPL == 1 ? UH : VPL == 2 ? 4 : 2; }
constexpr int arg_waves(int RL, int VPL) { return RL == 64 && VPL == 1 ? 16 : 4; }

template <int DT, int OP>
static void run(const ArgArgs& a, bool wide, hipStream_t s) {
    const ItemView& v = a.work;
    if (!wide) {
        launch_items<kWavesPerBlock>(k_seg_arg_narrow<DT, OP>, v.max_items, s, a.src, a.F, v.perm, v.begin, v.end,
                                     v.target, v.n_items, v.max_items, a.M, a.out, a.arg, a.partial, a.partial_arg);
    } else {
        for_row_shape<256>(a.F / 4, [&](auto rl, auto vpl) {
            constexpr int RL = decltype(rl)::value, VPL = decltype(vpl)::value, WPB = arg_waves(RL, VPL);
            constexpr int U = arg_rows_in_flight(RL, VPL, DT == HGNN_DT_I64 ? 8 : 16);
            launch_items<WPB>(k_seg_arg<DT, OP, RL, VPL, U, WPB>, v.max_items, s, a.src, a.F, a.F / 4, v.perm, v.begin,
                              v.end, v.target, v.n_items, v.max_items, a.M, a.out, a.arg, a.partial, a.partial_arg);
        });
    }
    const ItemView& c = a.split;
    launch_items<kWavesPerBlock>(k_arg_combine<DT, OP>, c.max_items, s, a.partial, a.partial_arg, a.F, c.target,
                                 c.begin, c.n_items, c.max_items, a.M, a.out, a.arg);
}

template <int DT>
static void run_minmax(const ArgArgs& a, int op, bool wide, hipStream_t s) {
    if (op == HGNN_RED_MIN) run<DT, HGNN_RED_MIN>(a, wide, s);
    else run<DT, HGNN_RED_MAX>(a, wide, s);
}

static int elem_bytes(int dtype) {
    switch (dtype) {
    case HGNN_DT_F32: return 4;
    case HGNN_DT_BF16: return 2;
    case HGNN_DT_I32: return 4;
    case HGNN_DT_I64: return 8;
    default: return 0;
    }
}

}  // namespace sarg
}  // namespace hgnn

using namespace hgnn;
using namespace hgnn::sarg;

extern "C" int hgnn_segment_reduce_ex(const hgnn_plan* plan, int32_t op, int32_t dtype, const void* src, int32_t F,
                                      void* out, int64_t* arg, void* partial, int32_t* partial_arg,
                                      hgnn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    HGNN_REQUIRE(op == HGNN_RED_SUM || op == HGNN_RED_MIN || op == HGNN_RED_MAX,
                 "hgnn_segment_reduce_ex: unknown op %d (HGNN_RED_SUM / _MIN / _MAX)", op);
    const int eb = elem_bytes(dtype);
    HGNN_REQUIRE(eb != 0, "hgnn_segment_reduce_ex: unknown dtype %d (HGNN_DT_F32 / _BF16 / _I32 / _I64)", dtype);
    if (op == HGNN_RED_SUM && (dtype == HGNN_DT_F32 || dtype == HGNN_DT_BF16)) {
        set_error("hgnn_segment_reduce_ex: floating-point sums are hgnn_segment_reduce_f32 / _bf16");
        return HGNN_ERR_UNSUPPORTED;
    }
    HGNN_REQUIRE(plan != nullptr, "hgnn_segment_reduce_ex: plan is NULL");
    HGNN_REQUIRE(F > 0, "hgnn_segment_reduce_ex: F must be positive (got %d)", F);
    HGNN_REQUIRE(!plan->has_gather, "hgnn_segment_reduce_ex: plan must be a plain destination plan (no gather index)");
    if (plan->n_dst == 0) return HGNN_OK;
    HGNN_REQUIRE(out != nullptr, "hgnn_segment_reduce_ex: out is NULL");
    HGNN_REQUIRE(op == HGNN_RED_SUM || arg != nullptr, "hgnn_segment_reduce_ex: arg is NULL");
    HGNN_REQUIRE(plan->n_rows == 0 || src != nullptr, "hgnn_segment_reduce_ex: src is NULL");
    HGNN_REQUIRE(plan->perm != nullptr || plan->n_rows == 0, "hgnn_segment_reduce_ex: plan->perm is NULL");
    HGNN_REQUIRE(plan->max_partial == 0 || (partial != nullptr && (op == HGNN_RED_SUM || partial_arg != nullptr)),
                 "hgnn_segment_reduce_ex: partial / partial_arg is NULL");
    // the 4-element column path needs every row start aligned to a 4-element group
    const uintptr_t al = (uintptr_t)(4 * eb < 16 ? 4 * eb : 16);
    const bool wide = F % 4 == 0 && F <= 1024 && (uintptr_t)src % al == 0 && (uintptr_t)out % al == 0 &&
                      (uintptr_t)partial % al == 0 && (uintptr_t)arg % 16 == 0 && (uintptr_t)partial_arg % 16 == 0;
    ArgArgs a = {src, F, plan->n_rows, out, arg, partial, partial_arg, work_items(plan), split_items(plan)};
    // position of sorted entry p = its row in src: perm[p], or p itself on an already sorted index
    if (plan->src_row == nullptr) a.work.perm = nullptr;
    if (op == HGNN_RED_SUM) {
        if (dtype == HGNN_DT_I32) run<HGNN_DT_I32, HGNN_RED_SUM>(a, wide, stream);
        else run<HGNN_DT_I64, HGNN_RED_SUM>(a, wide, stream);
    } else {
        switch (dtype) {
        case HGNN_DT_F32: run_minmax<HGNN_DT_F32>(a, op, wide, stream); break;
        case HGNN_DT_BF16: run_minmax<HGNN_DT_BF16>(a, op, wide, stream); break;
        case HGNN_DT_I32: run_minmax<HGNN_DT_I32>(a, op, wide, stream); break;
        default: run_minmax<HGNN_DT_I64>(a, op, wide, stream); break;
        }
    }
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}

extern "C" int hgnn_segment_arg_backward(const int64_t* arg, int64_t n_dst, int32_t F, int64_t n_rows, int32_t dtype,
                                         const void* grad_out, void* grad_src, hgnn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    HGNN_REQUIRE(dtype == HGNN_DT_F32 || dtype == HGNN_DT_BF16,
                 "hgnn_segment_arg_backward: dtype %d is not differentiable (HGNN_DT_F32 / _BF16)", dtype);
    HGNN_REQUIRE(n_dst >= 0 && n_rows >= 0 && F > 0, "hgnn_segment_arg_backward: bad sizes");
    if (n_rows == 0) return HGNN_OK;
    HGNN_REQUIRE(grad_src != nullptr, "hgnn_segment_arg_backward: grad_src is NULL");
    HGNN_REQUIRE(n_dst == 0 || (arg != nullptr && grad_out != nullptr), "hgnn_segment_arg_backward: NULL pointer");
    const int eb = elem_bytes(dtype);
    HGNN_CHECK_HIP(hipMemsetAsync(grad_src, 0, (size_t)n_rows * (size_t)F * (size_t)eb, stream));
    const int64_t total = n_dst * (int64_t)F;
    if (total > 0) {
        const unsigned blocks = capped_grid(ceil_div(total, kBlock));
        if (dtype == HGNN_DT_F32)
            k_arg_scatter<float><<<blocks, kBlock, 0, stream>>>(arg, (const float*)grad_out, total, F, n_rows,
                                                                (float*)grad_src);
        else
            k_arg_scatter<uint16_t><<<blocks, kBlock, 0, stream>>>(arg, (const uint16_t*)grad_out, total, F, n_rows,
                                                                   (uint16_t*)grad_src);
    }
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}
