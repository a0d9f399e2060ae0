// HBM-bound row kernels of the message-passing path (gfx950, wave64):
//
//   k_seg_reduce  : destination-sorted segmented reduce = scatter_add without atomics
//   k_seg_window  : the same for the headline shape (one 1-KiB row per wave instruction, no weight)
//                   (K1..K5: Modules/gnn_utils.py:50,124,125,142,143;
//                    BipartiteClassification/Models/HGNN_GMM.py:269)
//   k_gather_rows : out[e] = w[e]*rs[idx[e]]*table[idx[e]]   (K6 and scatter_add backward)
//   k_edge_dot    : out[e] = <A[ai[e]], B[bi[e]]>            (d/dweight of K2..K5)
//
// Layout: a feature row of F floats is read as F/4 float4 "columns".  RL lanes
// (a power of two, <= 64) cover one row with one 16-B load each, so a wave
// covers G = 64/RL rows per load instruction (F=256: one whole 1-KiB row per
// wave instruction, the widest coalesced access the hardware has).  Rows wider
// than 64 float4 use VPL loads per lane.  U independent row loads are issued
// before the first add so that each wave keeps U*G rows in flight.
//
// One wave owns one work item (= one destination, or one chunk of a long
// list): no atomics, every output row is written exactly once with 16-B
// stores, and the summation order is fixed by the plan.
#include "rows_common.h"

namespace hgnn {

int g_opt_nt_loads = 1;   // hgnn_set_option("nt_loads"): non-temporal loads for once-read source rows
int g_opt_nt_stores = 0;  // hgnn_set_option("nt_stores"): non-temporal stores for gather output
int g_opt_k1_one_launch = 1;  // hgnn_set_option("k1_one_launch"): the chunk that arrives last combines (_f32_ex)
int g_opt_k1_item_order = 0;  // hgnn_set_option("k1_item_order"): work items longest-first (_f32_ex); not shown to pay

// NT is a template parameter on purpose: written as `nt ? nontemporal_load(p) : *p` with a function argument,
// both arms load the same address, the helper is optimised before it is inlined, and the two loads are merged
// into one that keeps only the metadata they share, so the hint never reaches a caller.
template <bool NT>
__device__ __forceinline__ f32x4 ld4(const void* p) {
    if constexpr (NT) return __builtin_nontemporal_load((const f32x4*)p);
    else return *(const f32x4*)p;
}

// One launch per call (ItemExtra::arrive, rows_common.h): every lane of a wave calls this once its partial row p
// is stored.  True, wave-uniformly, in the chunk of split destination s that arrives last; it then sums the nch
// partial rows from pbegin on, in chunk order, into out[dst].  Nobody waits for anybody.
// The L2s of the eight XCDs are not coherent for plain accesses: the agent-scope release writes this wave's row
// back (stores drained first, and the write-back waited for by hand, which the compiler has been seen to skip),
// the acquire of the add drops this CU's stale lines before the rows of the other chunks are read.  The counter
// goes back to 0 for the next call, which is stream-ordered behind this one: no memset, and a captured graph
// replays.
__device__ __forceinline__ bool last_chunk_arrives(const ItemExtra& x, int p, int lane, int& pbegin, int& nch,
                                                   int& dst) {
    int s = 0, hi = min(*x.n_split, x.max_split);  // the last s with split_pbegin[s] <= p
    while (hi - s > 1) {
        const int mid = (s + hi) >> 1;
        if (x.split_pbegin[mid] <= p) s = mid;
        else hi = mid;
    }
    pbegin = x.split_pbegin[s];
    nch = x.split_pbegin[s + 1] - pbegin;
    dst = x.split_dst[s];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int seen = 0;
    if (lane == 0) seen = __hip_atomic_fetch_add(&x.arrive[s], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (__builtin_amdgcn_readfirstlane(seen) != nch - 1) return false;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) __hip_atomic_store(&x.arrive[s], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
}

// TAG distinguishes the main pass (0), the partial-sum combine pass (1) and the main pass on a
// destination-sorted index (2, identity row ids = streaming reads) in profiles.
template <int RL, int VPL, int U, bool HAS_W, bool HAS_RS, bool NT, int TAG, int WPB, bool XCD>
__global__ __launch_bounds__(WPB * 64) void k_seg_reduce(
    const float* __restrict__ src, int F, int nvec, const int32_t* __restrict__ src_row,
    const int32_t* __restrict__ perm, const float* __restrict__ weight,
    const float* __restrict__ row_scale, const int32_t* __restrict__ wi_begin,
    const int32_t* __restrict__ wi_end, const int32_t* __restrict__ wi_target,
    const int32_t* __restrict__ n_items_ptr, int64_t max_items, float* __restrict__ out,
    float* __restrict__ partial, ItemExtra x) {
    constexpr int G = 64 / RL;
    const int lane = threadIdx.x & 63;
    int64_t bid = blockIdx.x;
    if (XCD) {
        // blocks are dealt round-robin over the 8 XCDs: give each XCD a contiguous run of
        // work items so that neighbouring lists (which share index cache lines) share an L2.
        const int64_t per_xcd = (gridDim.x + 7) / 8;
        bid = (bid % 8) * per_xcd + bid / 8;
    }
    int64_t item = bid * WPB + (threadIdx.x >> 6);
    const int n_items = *n_items_ptr;
    if (item >= max_items) return;
    if (x.order != nullptr) item = x.order[item];  // slots past the count hold items past the count
    if (item >= n_items || item >= max_items) return;
    const int begin = __builtin_amdgcn_readfirstlane(wi_begin[item]);
    const int end = __builtin_amdgcn_readfirstlane(wi_end[item]);
    const int target = __builtin_amdgcn_readfirstlane(wi_target[item]);
    const int g = lane / RL;
    const int c = lane % RL;

    f32x4 acc[VPL];
#pragma unroll
    for (int v = 0; v < VPL; ++v) acc[v] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int base = begin; base < end; base += 64) {
        const int n = (end - base) < 64 ? (end - base) : 64;
        int my_row = 0;
        float my_w = 1.f;
        if (lane < n) {
            const int p = base + lane;
            my_row = src_row != nullptr ? src_row[p] : p;
            if (HAS_W) my_w = weight[perm != nullptr ? perm[p] : p];
            if (HAS_RS) my_w *= row_scale[my_row];
        }
        for (int j = 0; j < n; j += G * U) {
            f32x4 val[U][VPL];
            float w[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int e = j + u * G + g;
                int r;
                if (G == 1) {
                    r = __builtin_amdgcn_readlane(my_row, (j + u) & 63);
                    w[u] = (HAS_W || HAS_RS)
                               ? __builtin_bit_cast(float, __builtin_amdgcn_readlane(
                                                               __builtin_bit_cast(int, my_w), (j + u) & 63))
                               : 1.f;
                } else {
                    r = __shfl(my_row, e & 63);
                    w[u] = (HAS_W || HAS_RS) ? __shfl(my_w, e & 63) : 1.f;
                }
                const bool ok = e < n;
                const float* rp = src + (size_t)r * (size_t)F;
#pragma unroll
                for (int v = 0; v < VPL; ++v) {
                    const int cv = c + v * 64;
                    if (ok && cv < nvec)
                        val[u][v] = ld4<NT>(rp + cv * 4);
                    else
                        val[u][v] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int v = 0; v < VPL; ++v) {
                    if (HAS_W || HAS_RS)
                        acc[v] += val[u][v] * w[u];
                    else
                        acc[v] += val[u][v];
                }
            }
        }
    }
    if (G > 1) {
#pragma unroll
        for (int off = RL; off < 64; off <<= 1) {
#pragma unroll
            for (int v = 0; v < VPL; ++v) {
                acc[v].x += __shfl_xor(acc[v].x, off);
                acc[v].y += __shfl_xor(acc[v].y, off);
                acc[v].z += __shfl_xor(acc[v].z, off);
                acc[v].w += __shfl_xor(acc[v].w, off);
            }
        }
    }
    if (g == 0) {
        float* op = target >= 0 ? out + (size_t)target * (size_t)F
                                : partial + (size_t)(~target) * (size_t)F;
#pragma unroll
        for (int v = 0; v < VPL; ++v) {
            const int cv = c + v * 64;
            if (cv < nvec) *(f32x4*)(op + cv * 4) = acc[v];
        }
    }
    if constexpr (!HAS_W && !HAS_RS && TAG != 1) {
        if (x.arrive != nullptr && target < 0) {
            int pbegin, nch, dst;
            if (!last_chunk_arrives(x, ~target, lane, pbegin, nch, dst)) return;
#pragma unroll
            for (int v = 0; v < VPL; ++v) acc[v] = f32x4{0.f, 0.f, 0.f, 0.f};
            // the order of the TAG 1 launch, bit for bit: lane group g adds the partial rows g, g + G, .. in
            // chunk order, then the groups are added as above
            for (int k = g; k < nch; k += G) {
                const float* rp = partial + (size_t)(pbegin + k) * (size_t)F;
#pragma unroll
                for (int v = 0; v < VPL; ++v) {
                    const int cv = c + v * 64;
                    if (cv < nvec) acc[v] += ld4<NT>(rp + cv * 4);
                }
            }
            if (G > 1) {
#pragma unroll
                for (int off = RL; off < 64; off <<= 1) {
#pragma unroll
                    for (int v = 0; v < VPL; ++v) {
                        acc[v].x += __shfl_xor(acc[v].x, off);
                        acc[v].y += __shfl_xor(acc[v].y, off);
                        acc[v].z += __shfl_xor(acc[v].z, off);
                        acc[v].w += __shfl_xor(acc[v].w, off);
                    }
                }
            }
            float* op = out + (size_t)dst * (size_t)F;
#pragma unroll
            for (int v = 0; v < VPL; ++v) {
                const int cv = c + v * 64;
                if (g == 0 && cv < nvec) *(f32x4*)(op + cv * 4) = acc[v];
            }
        }
    }
}

// The headline shape (one 1-KiB row per wave instruction, no weight, no row scale): a rolling window of W row
// loads per wave.  After the prologue the oldest row is added and the load of row i+W is issued into the slot it
// frees, so inside the steady loop (lists of 2W rows and more) the wave waits with a counted vmcnt(W-1).
// Everything that decides control flow is wave-uniform (the work item comes in by scalar loads, read before the
// item count is known), so no load sits behind an exec-mask branch.  A ragged end is issued as groups of W/2,
// W/4, .. 1 rows into slots the drain has added.  That part is NOT overlapped in the main pass as compiled: the
// conditional overwrite of the last slots makes the compiler copy them first, so a list of W+1..2W-1 rows waits
// for W-1 of its W loads before its first ragged load goes out (two memory latencies, as in k_seg_reduce); the
// sorted-layout and combine instantiations drain with vmcnt(W-1), W-2, ..  
// Rows are added one by one in list order, starting from 0: the sum is bitwise the one of k_seg_reduce.
// TAG 0 reads its rows through src_row; TAG 1 (combine) and TAG 2 (sorted layout) read rows begin..end-1.
// Reads before the count is known: wi_begin, wi_end and wi_target need max_items entries each (the combine pass:
// split_items, rows_common.h).
template <int W, bool NT, int TAG, int WPB>
__global__ __launch_bounds__(WPB * 64) void k_seg_window(
    const float* __restrict__ src, int F, int nvec, const int32_t* __restrict__ src_row,
    const int32_t* __restrict__ wi_begin, const int32_t* __restrict__ wi_end,
    const int32_t* __restrict__ wi_target, const int32_t* __restrict__ n_items_ptr, int64_t max_items,
    float* __restrict__ out, float* __restrict__ partial, ItemExtra x) {
    static_assert(W >= 2 && 64 % W == 0, "a 64-row trip is a whole number of windows");
    constexpr bool IDENT = TAG != 0;
    const int lane = threadIdx.x & 63;
    int64_t item = (int64_t)blockIdx.x * WPB + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (item >= max_items) return;
    // longest lists first (hgnn_plan_item_order): one more scalar load at the head of the chain.  A slot past
    // the count holds an item past the count; the clamp only keeps a foreign `order` inside the arrays.
    if (x.order != nullptr) item = x.order[item];
    // four scalar loads issued together: an item past the count (known only now) becomes an empty list that
    // stores nothing, so that none of the loads can be moved behind a branch on the count
    const bool valid = item < *n_items_ptr;
    item = item < max_items ? item : max_items - 1;
    const int begin = wi_begin[item];
    const int end = begin + (int)(((uint32_t)wi_end[item] - (uint32_t)begin) & (valid ? ~0u : 0u));
    const int target = wi_target[item];
    // lanes past the row's last float4 (F < 256) re-read column 0 and store nothing
    const uint32_t voff = (uint32_t)(lane < nvec ? lane : 0) * 16u;
    const size_t row_bytes = (size_t)F * sizeof(float);

    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 ring[W];
    int ids = 0, ids_next = 0;
    if (!IDENT && begin < end) ids_next = src_row[min(begin + lane, end - 1)];
    for (int base = begin; base < end; base += 64) {
        const int n = min(end - base, 64);
        if (!IDENT) {
            // the next trip's row ids are on their way while this trip's rows stream
            ids = ids_next;
            if (base + 64 < end) ids_next = src_row[min(base + 64 + lane, end - 1)];
        }
        auto row = [&](int j) -> f32x4 {  // j: wave-uniform position in this trip
            const uint32_t r = IDENT ? (uint32_t)(base + j) : (uint32_t)__builtin_amdgcn_readlane(ids, j);
            return ld4<NT>((const char*)src + (size_t)r * row_bytes + voff);
        };
        const int full = n & ~(W - 1), rem = n & (W - 1);
        const bool have = full > 0;  // a list shorter than W goes straight to its ragged end
        if (have) {
#pragma unroll
            for (int u = 0; u < W; ++u) ring[u] = row(u);
        }
        for (int j = W; j < full; j += W) {
#pragma unroll
            for (int u = 0; u < W; ++u) {
                acc += ring[u];
                ring[u] = row(j + u);
                __builtin_amdgcn_sched_barrier(0);  // keep add-oldest-then-issue order: the wait stays vmcnt(W-1)
            }
        }
        // drain the last whole window; each group of the ragged end goes into slots already added
        int j = full;
#pragma unroll
        for (int g = W / 2, o = 0; g >= 1; o += g, g >>= 1) {
            if (have) {
#pragma unroll
                for (int k = 0; k < g; ++k) acc += ring[o + k];
            }
            __builtin_amdgcn_sched_barrier(0);
            if (rem & g) {
#pragma unroll
                for (int k = 0; k < g; ++k) ring[o + k] = row(j + k);
                j += g;
            }
        }
        if (have) acc += ring[W - 1];
#pragma unroll
        for (int g = W / 2, o = 0; g >= 1; o += g, g >>= 1) {
            if (rem & g) {
#pragma unroll
                for (int k = 0; k < g; ++k) acc += ring[o + k];
            }
        }
    }
    float* op = target >= 0 ? out + (size_t)target * (size_t)F : partial + (size_t)(~target) * (size_t)F;
    if (valid && lane < nvec) *(f32x4*)(op + lane * 4) = acc;
    if constexpr (TAG != 1) {
        if (x.arrive != nullptr && valid && target < 0) {
            int pbegin, nch, dst;
            if (!last_chunk_arrives(x, ~target, lane, pbegin, nch, dst)) return;
            // four partial rows in flight; kept below the eight loads of a window on purpose
            const char* pp = (const char*)partial + (size_t)pbegin * row_bytes + voff;
            acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
            for (int k = 0; k < nch; k += 4) {
                f32x4 part[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) part[u] = ld4<NT>(pp + (size_t)min(k + u, nch - 1) * row_bytes);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (k + u < nch) acc += part[u];
                }
            }
            if (lane < nvec) *(f32x4*)(out + (size_t)dst * (size_t)F + lane * 4) = acc;
        }
    }
}

// any F (including F % 4 != 0): lanes stride over single floats, 64 columns per pass.
template <bool HAS_W, bool HAS_RS>
__global__ __launch_bounds__(256) void k_seg_reduce_scalar(
    const float* __restrict__ src, int F, const int32_t* __restrict__ src_row,
    const int32_t* __restrict__ perm, const float* __restrict__ weight,
    const float* __restrict__ row_scale, const int32_t* __restrict__ wi_begin,
    const int32_t* __restrict__ wi_end, const int32_t* __restrict__ wi_target,
    const int32_t* __restrict__ n_items_ptr, int64_t max_items, float* __restrict__ out,
    float* __restrict__ partial) {
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int n_items = *n_items_ptr;
    if (item >= n_items || item >= max_items) return;
    const int begin = wi_begin[item], end = wi_end[item], target = wi_target[item];
    float* op = target >= 0 ? out + (size_t)target * (size_t)F : partial + (size_t)(~target) * (size_t)F;
    for (int col0 = 0; col0 < F; col0 += 64) {
        const int col = col0 + lane;
        float acc = 0.f;
        for (int p = begin; p < end; ++p) {
            const int r = src_row != nullptr ? src_row[p] : p;
            float w = 1.f;
            if (HAS_W) w = weight[perm != nullptr ? perm[p] : p];
            if (HAS_RS) w *= row_scale[r];
            if (col < F) acc += w * src[(size_t)r * (size_t)F + col];
        }
        if (col < F) op[col] = acc;
    }
}

template <int RL, int VPL, int U, bool HAS_W, bool HAS_RS>
__global__ __launch_bounds__(256) void k_gather_rows(const float* __restrict__ table, int F, int nvec,
                                                     const int32_t* __restrict__ idx, int64_t M,
                                                     const float* __restrict__ weight,
                                                     const float* __restrict__ row_scale,
                                                     float* __restrict__ out, bool nt_store) {
    constexpr int G = 64 / RL;
    const int lane = threadIdx.x & 63;
    const int g = lane / RL;
    const int c = lane % RL;
    const int64_t n_tiles = (M + 63) / 64;
    for (int64_t tile = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); tile < n_tiles;
         tile += (int64_t)gridDim.x * kWavesPerBlock) {
        const int64_t base = tile * 64;
        const int n = (M - base) < 64 ? (int)(M - base) : 64;
        int my_idx = -1;
        float my_w = 1.f;
        if (lane < n) {
            my_idx = idx[base + lane];
            if (HAS_W) my_w = weight[base + lane];
            if (HAS_RS) my_w *= my_idx >= 0 ? row_scale[my_idx] : 0.f;
        }
        for (int j = 0; j < n; j += G * U) {
            f32x4 val[U][VPL];
            float w[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int e = j + u * G + g;
                const int r = __shfl(my_idx, e & 63);
                w[u] = (HAS_W || HAS_RS) ? __shfl(my_w, e & 63) : 1.f;
                const bool ok = (e < n) && (r >= 0);
                const float* rp = table + (size_t)(ok ? r : 0) * (size_t)F;
#pragma unroll
                for (int v = 0; v < VPL; ++v) {
                    const int cv = c + v * 64;
                    if (ok && cv < nvec)
                        val[u][v] = *(const f32x4*)(rp + cv * 4);
                    else
                        val[u][v] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int e = j + u * G + g;
                if (e < n) {
                    float* op = out + (size_t)(base + e) * (size_t)F;
#pragma unroll
                    for (int v = 0; v < VPL; ++v) {
                        const int cv = c + v * 64;
                        if (cv < nvec) {
                            f32x4 x = (HAS_W || HAS_RS) ? val[u][v] * w[u] : val[u][v];
                            if (nt_store)
                                __builtin_nontemporal_store(x, (f32x4*)(op + cv * 4));
                            else
                                *(f32x4*)(op + cv * 4) = x;
                        }
                    }
                }
            }
        }
    }
}

// Transpose of k_seg_reduce: walk the plan in destination order, read each table row once and
// write it (scaled) to every row of its list.  out[perm[p],:] = w[perm[p]] * table[dst,:].
template <int RL, int VPL, bool HAS_W, int WPB>
__global__ __launch_bounds__(WPB * 64) void k_spread_rows(
    const float* __restrict__ table, int F, int nvec, const int32_t* __restrict__ perm,
    const float* __restrict__ weight, const int32_t* __restrict__ wi_begin,
    const int32_t* __restrict__ wi_end, const int32_t* __restrict__ wi_dst,
    const int32_t* __restrict__ n_items_ptr, int64_t max_items, float* __restrict__ out, bool nt_store) {
    constexpr int G = 64 / RL;
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
    const int n_items = *n_items_ptr;
    if (item >= n_items || item >= max_items) return;
    const int begin = __builtin_amdgcn_readfirstlane(wi_begin[item]);
    const int end = __builtin_amdgcn_readfirstlane(wi_end[item]);
    if (begin >= end) return;
    const int dst = __builtin_amdgcn_readfirstlane(wi_dst[item]);
    const int g = lane / RL;
    const int c = lane % RL;
    f32x4 row[VPL];
    const float* rp = table + (size_t)dst * (size_t)F;
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
        const int cv = c + v * 64;
        row[v] = cv < nvec ? *(const f32x4*)(rp + cv * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int base = begin; base < end; base += 64) {
        const int n = (end - base) < 64 ? (end - base) : 64;
        int my_e = 0;
        float my_w = 1.f;
        if (lane < n) {
            my_e = perm[base + lane];
            if (HAS_W) my_w = weight[my_e];
        }
        for (int j = 0; j < n; j += G) {
            const int k = j + g;
            const int e = __shfl(my_e, k & 63);
            const float w = HAS_W ? __shfl(my_w, k & 63) : 1.f;
            if (k < n) {
                float* op = out + (size_t)e * (size_t)F;
#pragma unroll
                for (int v = 0; v < VPL; ++v) {
                    const int cv = c + v * 64;
                    if (cv < nvec) {
                        const f32x4 x = HAS_W ? row[v] * w : row[v];
                        if (nt_store)
                            __builtin_nontemporal_store(x, (f32x4*)(op + cv * 4));
                        else
                            *(f32x4*)(op + cv * 4) = x;
                    }
                }
            }
        }
    }
}

template <bool HAS_W>
__global__ __launch_bounds__(256) void k_spread_rows_scalar(
    const float* __restrict__ table, int F, const int32_t* __restrict__ perm,
    const float* __restrict__ weight, const int32_t* __restrict__ wi_begin,
    const int32_t* __restrict__ wi_end, const int32_t* __restrict__ wi_dst,
    const int32_t* __restrict__ n_items_ptr, int64_t max_items, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int n_items = *n_items_ptr;
    if (item >= n_items || item >= max_items) return;
    const int begin = wi_begin[item], end = wi_end[item], dst = wi_dst[item];
    for (int p = begin; p < end; ++p) {
        const int e = perm[p];
        const float w = HAS_W ? weight[e] : 1.f;
        for (int col = lane; col < F; col += 64)
            out[(size_t)e * F + col] = w * table[(size_t)dst * F + col];
    }
}

template <bool HAS_W, bool HAS_RS>
__global__ __launch_bounds__(256) void k_gather_rows_scalar(const float* __restrict__ table, int F,
                                                            const int32_t* __restrict__ idx, int64_t M,
                                                            const float* __restrict__ weight,
                                                            const float* __restrict__ row_scale,
                                                            float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    for (int64_t e = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); e < M;
         e += (int64_t)gridDim.x * kWavesPerBlock) {
        const int r = idx[e];
        float w = 1.f;
        if (HAS_W) w = weight[e];
        if (HAS_RS) w *= r >= 0 ? row_scale[r] : 0.f;
        for (int col = lane; col < F; col += 64)
            out[(size_t)e * F + col] = r >= 0 ? w * table[(size_t)r * F + col] : 0.f;
    }
}

template <int RL, int VPL>
__global__ __launch_bounds__(256) void k_edge_dot(const float* __restrict__ A, const int32_t* __restrict__ ai,
                                                  const float* __restrict__ B, const int32_t* __restrict__ bi,
                                                  int F, int nvec, int64_t M, float* __restrict__ out) {
    constexpr int G = 64 / RL;
    const int lane = threadIdx.x & 63;
    const int g = lane / RL;
    const int c = lane % RL;
    const int64_t n_tiles = (M + 63) / 64;
    for (int64_t tile = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); tile < n_tiles;
         tile += (int64_t)gridDim.x * kWavesPerBlock) {
        const int64_t base = tile * 64;
        const int n = (M - base) < 64 ? (int)(M - base) : 64;
        int my_a = -1, my_b = -1;
        if (lane < n) {
            my_a = ai != nullptr ? ai[base + lane] : (int)(base + lane);
            my_b = bi != nullptr ? bi[base + lane] : (int)(base + lane);
        }
        for (int j = 0; j < n; j += G * 2) {
            float s[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int e = j + u * G + g;
                const int ra = __shfl(my_a, e & 63);
                const int rb = __shfl(my_b, e & 63);
                const bool ok = (e < n) && ra >= 0 && rb >= 0;
                s[u] = 0.f;
                const float* pa = A + (size_t)(ok ? ra : 0) * (size_t)F;
                const float* pb = B + (size_t)(ok ? rb : 0) * (size_t)F;
#pragma unroll
                for (int v = 0; v < VPL; ++v) {
                    const int cv = c + v * 64;
                    if (ok && cv < nvec) {
                        f32x4 x = *(const f32x4*)(pa + cv * 4);
                        f32x4 y = *(const f32x4*)(pb + cv * 4);
                        s[u] += x.x * y.x + x.y * y.y + x.z * y.z + x.w * y.w;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                float t = s[u];
#pragma unroll
                for (int off = 1; off < RL; off <<= 1) t += __shfl_xor(t, off);
                const int e = j + u * G + g;
                if (c == 0 && e < n) out[base + e] = t;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_edge_dot_scalar(const float* __restrict__ A, const int32_t* __restrict__ ai,
                                                         const float* __restrict__ B, const int32_t* __restrict__ bi,
                                                         int F, int64_t M, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    for (int64_t e = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); e < M;
         e += (int64_t)gridDim.x * kWavesPerBlock) {
        const int ra = ai != nullptr ? ai[e] : (int)e;
        const int rb = bi != nullptr ? bi[e] : (int)e;
        float t = 0.f;
        if (ra >= 0 && rb >= 0)
            for (int col = lane; col < F; col += 64) t += A[(size_t)ra * F + col] * B[(size_t)rb * F + col];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) t += __shfl_xor(t, off);
        if (lane == 0) out[e] = t;
    }
}

// ------------------------------------------------------------------ dispatch
struct SegArgs {
    const float* src;
    int F;
    const float* weight;
    const float* row_scale;
    float *out, *partial;
    ItemView items;
    ItemExtra extra;  // zeros: plan order, combine by a second launch
};

// The one place that decides on non-temporal row loads: fn(bool_constant<NT>).  The partial rows of the combine
// pass (TAG 1) were just written and are small: they are read with plain loads, and no NT kernel exists for them.
template <int TAG, class Fn>
static void with_nt_loads(Fn&& fn) {
    if constexpr (TAG != 1) {
        if (g_opt_nt_loads) return fn(std::true_type{});
    }
    fn(std::false_type{});
}

template <int RL, int VPL, int U, bool W, bool RS, bool NT, int TAG, int WPB>
static void launch_seg3(const SegArgs& a, hipStream_t s) {
    const ItemView& v = a.items;
    launch_items<WPB>(k_seg_reduce<RL, VPL, U, W, RS, NT, TAG, WPB, false>, v.max_items, s, a.src, a.F, a.F / 4,
                      v.src_row, v.perm, a.weight, a.row_scale, v.begin, v.end, v.target, v.n_items, v.max_items,
                      a.out, a.partial, a.extra);
}

template <int RL, int VPL, int U, bool W, bool RS, int TAG>
static void launch_seg(const SegArgs& a, hipStream_t s) {
    with_nt_loads<TAG>([&](auto nt) { launch_seg3<RL, VPL, U, W, RS, decltype(nt)::value, TAG, 4>(a, s); });
}

template <int W, bool NT, int TAG, int WPB>
static void launch_window(const SegArgs& a, hipStream_t s) {
    const ItemView& v = a.items;
    launch_items<WPB>(k_seg_window<W, NT, TAG, WPB>, v.max_items, s, a.src, a.F, a.F / 4, v.src_row, v.begin, v.end,
                      v.target, v.n_items, v.max_items, a.out, a.partial, a.extra);
}

#ifdef HGNN_K1_SWEEP
// tools/tune_k1_window.py builds a library of its own with every variant and picks one through hgnn_set_option
int g_opt_k1_window = 16, g_opt_k1_waves = 8;
#endif

// 1-KiB rows (F in (128, 256], the headline shape) without weight: k_seg_window, a window of 16 rows per wave, 8 waves
// per workgroup, non-temporal row loads (sweep of window depth x waves x nt: tools/tune_k1_window.py, DESIGN.md
// section 3).  An XCD-contiguous remap of the work items was 3-4 % slower (profiles/r01_tune_k1_L256.txt).
template <int TAG>
static void launch_seg_headline(const SegArgs& a, hipStream_t s) {
    with_nt_loads<TAG>([&](auto nt) {
        constexpr bool NT = decltype(nt)::value;
#ifdef HGNN_K1_SWEEP
        auto waves = [&](auto w) {
            constexpr int W = decltype(w)::value;
            if (g_opt_k1_waves == 4) launch_window<W, NT, TAG, 4>(a, s);
            else if (g_opt_k1_waves == 8) launch_window<W, NT, TAG, 8>(a, s);
            else launch_window<W, NT, TAG, 16>(a, s);
        };
        // window 0 = control: the burst-then-drain kernel this one replaced, with a real nt hint
        if (g_opt_k1_window == 0) launch_seg3<64, 1, 16, false, false, NT, TAG, 16>(a, s);
        else if (g_opt_k1_window == 8) waves(std::integral_constant<int, 8>{});
        else if (g_opt_k1_window == 32) waves(std::integral_constant<int, 32>{});
        else waves(std::integral_constant<int, 16>{});
#else
        launch_window<16, NT, TAG, 8>(a, s);
#endif
    });
}

// rows in flight per wave, by row shape  (RL 32: U8 / 16-wave variants were within 1 %)
constexpr int seg_rows_in_flight(int RL, int VPL) { return RL < 64 ? 4 : VPL == 1 ? 8 : VPL == 2 ? 4 : 2; }

template <bool W, bool RS, int TAG>
static void dispatch_seg(const SegArgs& a, hipStream_t s) {
    const ItemView& v = a.items;
    if (a.F % 4 != 0 || a.F > 1024)
        return launch_items<kWavesPerBlock>(k_seg_reduce_scalar<W, RS>, v.max_items, s, a.src, a.F, v.src_row, v.perm,
                                            a.weight, a.row_scale, v.begin, v.end, v.target, v.n_items, v.max_items,
                                            a.out, a.partial);
    for_row_shape<256>(a.F / 4, [&](auto rl, auto vpl) {
        constexpr int RL = decltype(rl)::value, VPL = decltype(vpl)::value;
        if constexpr (RL == 64 && VPL == 1 && !W && !RS) launch_seg_headline<TAG>(a, s);
        else launch_seg<RL, VPL, seg_rows_in_flight(RL, VPL), W, RS, TAG>(a, s);
    });
}

}  // namespace hgnn

using namespace hgnn;

// `who` names the entry point in error messages.  arrive == NULL: the combine pass is a second launch.
static int segment_reduce_f32(const char* who, const hgnn_plan* plan, const float* src, int32_t F,
                              const float* weight, const float* row_scale, float* out, float* partial,
                              int32_t* arrive, const int32_t* order, hipStream_t stream) {
    HGNN_REQUIRE(plan != nullptr, "%s: plan is NULL", who);
    HGNN_REQUIRE(F > 0, "%s: F must be positive (got %d)", who, F);
    if (plan->n_dst == 0) return HGNN_OK;
    HGNN_REQUIRE(out != nullptr, "%s: out is NULL", who);
    HGNN_REQUIRE(plan->n_rows == 0 || src != nullptr, "%s: src is NULL", who);
    HGNN_REQUIRE(plan->src_row != nullptr || !plan->has_gather,
                 "%s: src_row may only be NULL for a sorted plan without gather", who);
    HGNN_REQUIRE(partial != nullptr || plan->max_partial == 0, "%s: partial is NULL", who);
    HGNN_REQUIRE(((uintptr_t)src % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)partial % 16 == 0) || F % 4 != 0,
                 "%s: src/out/partial must be 16-byte aligned", who);
    SegArgs a = {src, F, weight, row_scale, out, partial, work_items(plan), ItemExtra{}};
    // the in-kernel combine and the item order exist in the plain fp32 vector kernels only
    const bool plain_vec = !weight && !row_scale && F % 4 == 0 && F <= 1024;
    const bool one_launch = plain_vec && arrive != nullptr && g_opt_k1_one_launch;
    if (plain_vec) a.extra = item_extra(plan, g_opt_k1_item_order ? order : nullptr, one_launch ? arrive : nullptr);
    if (weight && row_scale) dispatch_seg<true, true, 0>(a, stream);
    else if (weight) dispatch_seg<true, false, 0>(a, stream);
    else if (row_scale) {
        set_error("%s: row_scale requires weight", who);
        return HGNN_ERR_UNSUPPORTED;
    } else if (plan->src_row == nullptr) {
        dispatch_seg<false, false, 2>(a, stream);  // TAG 2: sorted-layout (streaming) launches, named apart in profiles
    } else dispatch_seg<false, false, 0>(a, stream);
    // second pass: sum the partial rows of split destinations, in chunk order
    if (!one_launch)
        dispatch_seg<false, false, 1>(
            SegArgs{partial, F, nullptr, nullptr, out, partial, split_items(plan), ItemExtra{}}, stream);
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}

extern "C" int hgnn_segment_reduce_f32(const hgnn_plan* plan, const float* src, int32_t F,
                                       const float* weight, const float* row_scale, float* out,
                                       float* partial, hgnn_stream_t stream) {
    return segment_reduce_f32("hgnn_segment_reduce_f32", plan, src, F, weight, row_scale, out, partial, nullptr,
                              nullptr, (hipStream_t)stream);
}

extern "C" int hgnn_segment_reduce_f32_ex(const hgnn_plan* plan, const float* src, int32_t F,
                                          const float* weight, const float* row_scale, float* out,
                                          float* partial, int32_t* arrive, const int32_t* order,
                                          hgnn_stream_t stream) {
    HGNN_REQUIRE(plan == nullptr || arrive != nullptr, "hgnn_segment_reduce_f32_ex: arrive is NULL");
    return segment_reduce_f32("hgnn_segment_reduce_f32_ex", plan, src, F, weight, row_scale, out, partial, arrive,
                              order, (hipStream_t)stream);
}

constexpr int gather_rows_in_flight(int RL, int VPL) { return RL <= 8 ? 2 : RL < 64 ? 4 : VPL == 1 ? 8 : VPL == 2 ? 4 : 2; }

template <bool W, bool RS>
static void dispatch_gather(const float* table, int F, const int32_t* idx, int64_t M, const float* weight,
                            const float* row_scale, float* out, hipStream_t s) {
    if (F % 4 != 0 || F > 1024) {
        k_gather_rows_scalar<W, RS><<<stream_grid(M), kBlock, 0, s>>>(table, F, idx, M, weight, row_scale, out);
        return;
    }
    const unsigned grid = stream_grid(ceil_div(M, 64));
    const bool nt = g_opt_nt_stores != 0;
    for_row_shape<256>(F / 4, [&](auto rl, auto vpl) {
        constexpr int RL = decltype(rl)::value, VPL = decltype(vpl)::value;
        k_gather_rows<RL, VPL, gather_rows_in_flight(RL, VPL), W, RS><<<grid, kBlock, 0, s>>>(
            table, F, F / 4, idx, M, weight, row_scale, out, nt);
    });
}

extern "C" int hgnn_gather_rows_f32(const float* table, int64_t table_rows, int32_t F, const int32_t* idx,
                                    int64_t M, const float* weight, const float* row_scale, float* out,
                                    hgnn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    HGNN_REQUIRE(F > 0 && M >= 0 && table_rows >= 0, "hgnn_gather_rows_f32: bad sizes");
    if (M == 0) return HGNN_OK;
    HGNN_REQUIRE(table != nullptr && idx != nullptr && out != nullptr, "hgnn_gather_rows_f32: NULL pointer");
    HGNN_REQUIRE(((uintptr_t)table % 16 == 0 && (uintptr_t)out % 16 == 0) || F % 4 != 0,
                 "hgnn_gather_rows_f32: table/out must be 16-byte aligned");
    if (weight && row_scale) dispatch_gather<true, true>(table, F, idx, M, weight, row_scale, out, stream);
    else if (weight) dispatch_gather<true, false>(table, F, idx, M, weight, row_scale, out, stream);
    else if (row_scale) dispatch_gather<false, true>(table, F, idx, M, weight, row_scale, out, stream);
    else dispatch_gather<false, false>(table, F, idx, M, weight, row_scale, out, stream);
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}

constexpr int spread_waves(int RL) { return RL < 64 ? 4 : 8; }  // per workgroup

template <bool W>
static void dispatch_spread(const ItemView& v, const float* table, int F, const float* weight, float* out,
                            hipStream_t s) {
    if (F % 4 != 0 || F > 1024)
        return launch_items<kWavesPerBlock>(k_spread_rows_scalar<W>, v.max_items, s, table, F, v.perm, weight, v.begin,
                                            v.end, v.wi_dst, v.n_items, v.max_items, out);
    const bool nt = g_opt_nt_stores != 0;
    for_row_shape<256>(F / 4, [&](auto rl, auto vpl) {
        constexpr int RL = decltype(rl)::value, VPL = decltype(vpl)::value, WPB = spread_waves(RL);
        launch_items<WPB>(k_spread_rows<RL, VPL, W, WPB>, v.max_items, s, table, F, F / 4, v.perm, weight, v.begin,
                          v.end, v.wi_dst, v.n_items, v.max_items, out, nt);
    });
}

extern "C" int hgnn_spread_rows_f32(const hgnn_plan* plan, const float* table, int32_t F, const float* weight,
                                    float* out, hgnn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    HGNN_REQUIRE(plan != nullptr, "hgnn_spread_rows_f32: plan is NULL");
    HGNN_REQUIRE(F > 0, "hgnn_spread_rows_f32: F must be positive");
    if (plan->n_rows == 0 || plan->n_dst == 0) return HGNN_OK;
    HGNN_REQUIRE(!plan->has_gather, "hgnn_spread_rows_f32: plan must be a plain destination plan");
    HGNN_REQUIRE(table != nullptr && out != nullptr, "hgnn_spread_rows_f32: NULL pointer");
    HGNN_REQUIRE(((uintptr_t)table % 16 == 0 && (uintptr_t)out % 16 == 0) || F % 4 != 0,
                 "hgnn_spread_rows_f32: table/out must be 16-byte aligned");
    if (weight) dispatch_spread<true>(work_items(plan), table, F, weight, out, stream);
    else dispatch_spread<false>(work_items(plan), table, F, weight, out, stream);
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}

extern "C" int hgnn_edge_dot_f32(const float* A, const int32_t* ai, int64_t a_rows, const float* B,
                                 const int32_t* bi, int64_t b_rows, int32_t F, int64_t M, float* out,
                                 hgnn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    HGNN_REQUIRE(F > 0 && M >= 0, "hgnn_edge_dot_f32: bad sizes");
    if (M == 0) return HGNN_OK;
    HGNN_REQUIRE(A != nullptr && B != nullptr && out != nullptr, "hgnn_edge_dot_f32: NULL pointer");
    HGNN_REQUIRE((ai != nullptr || a_rows >= M) && (bi != nullptr || b_rows >= M),
                 "hgnn_edge_dot_f32: identity-indexed operand has fewer than M rows");
    if (F % 4 != 0 || F > 1024 || (uintptr_t)A % 16 != 0 || (uintptr_t)B % 16 != 0) {
        k_edge_dot_scalar<<<stream_grid(M), kBlock, 0, stream>>>(A, ai, B, bi, F, M, out);
    } else {
        const unsigned grid = stream_grid(ceil_div(M, 64));
        for_row_shape<256>(F / 4, [&](auto rl, auto vpl) {
            k_edge_dot<decltype(rl)::value, decltype(vpl)::value><<<grid, kBlock, 0, stream>>>(A, ai, B, bi, F, F / 4, M,
                                                                                              out);
        });
    }
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}
