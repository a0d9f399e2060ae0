// k_tp_*: EmbeddingBase.get_training_samples (reference GNNEmbedding/embedding_base.py:109-135) from the kNN matrix
// idx int64 [N, K <= 128] straight to (new_graph, y), without the [2, N*K] prediction graph and without a sort of
// the pairs.  Everything the function decides about a pair (i, j) is local to row i of idx:
//
//   e_bidir  = [mte, mte.flip(0)] restricted to the columns whose two ends pass signal_mask, original order
//   modulewise  row i emits its DISTINCT valid ids j ascending where (i, j) is not in e_bidir and
//               (pid[i] != pid[j] || pid[i] == 0 || pid[j] == 0), y = 0; then all of e_bidir, y = 1
//   pid         row i emits every valid slot in slot order where !(signal[i] && signal[j]) and
//               !(pid[i] == pid[j] && both != 0), y = 0; the e_bidir part is empty (its pairs pass the signal mask)
//
// Data flow (every array in the workspace):
//
//   k_tp_truth     one thread per column of [mte, mte.flip(0)]: the keep flag into counts[N + c] and, modulewise, the
//                  key row << 31 | col (a sentinel that sorts last when not kept); an id outside [0, N) sets the status
//   radix sort     rocprim::radix_sort_keys of those <= 2T keys (modulewise), once per call
//   k_tp_rowstart  one lower bound per row: rowstart[i] = first sorted key of row i, i in [0, N]
//   k_tp_rows      ONE WAVE PER ROW, a lane holds slots lane and lane + 64.  Modulewise: a shuffle bitonic network
//                  sorts the row's ids in registers (empty slots and bad ids are a sentinel that sorts last), a slot
//                  equal to its predecessor is dropped, and a lane looks its id up in the row's run of sorted keys.
//                  Ranks: __ballot and a popcount of the lower lanes.  COUNT writes counts[i]
//   exclusive scan rocprim, int32, over counts[N + 2T] -> offs: every output position
//   k_tp_info      {P, n_row_part, n_truth_part, status} into the caller's device int64[4]: the ONE host read
//   k_tp_rows FILL the same decisions again (no per-pair flags are stored), written at offs[i] + rank
//   k_tp_truth_fill  the kept columns of [mte, mte.flip(0)] at offs[N + c], y = 1
//
// No atomic decides a position (the order is fixed); the only atomic is an integer OR into the status word.  An id
// is compared with its range before it forms an address.  No LDS, no scratch memory.
#include "common.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace hgnn {
namespace {

constexpr int kTpIdBits = 31;
constexpr unsigned kTpKeyBits = 2 * kTpIdBits + 1;           // the sentinel's bit included
constexpr uint64_t kTpNoKey = (uint64_t)1 << (2 * kTpIdBits);   // above every row << 31 | col
constexpr int32_t kTpNoId = 0x7fffffff;                      // above every id: N <= 2^31 - 1
constexpr int64_t kTpMaxN = ((int64_t)1 << 31) - 1;
constexpr int64_t kTpMaxBlocks = 16384;

struct TpWorkspace {
    size_t counts, offs, status, tkey, tkey_s, rowstart, temp, temp_bytes, total;
};

int tp_layout(int64_t N, int64_t T, bool modulewise, TpWorkspace* w, hipStream_t stream) {
    size_t t1 = 0, t2 = 0;
    const size_t L = (size_t)N + 2 * (size_t)T, t2x = 2 * (size_t)T;
    if (L > 0)
        HGNN_CHECK_HIP(rocprim::exclusive_scan(nullptr, t1, (int32_t*)nullptr, (int32_t*)nullptr, (int32_t)0, L,
                                               rocprim::plus<int32_t>(), stream));
    if (modulewise && T > 0)
        HGNN_CHECK_HIP(rocprim::radix_sort_keys(nullptr, t2, (uint64_t*)nullptr, (uint64_t*)nullptr, t2x, 0u,
                                                kTpKeyBits, stream));
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    };
    w->counts = take(L * 4);
    w->offs = take(L * 4);
    w->status = take(sizeof(int32_t));
    w->tkey = take(modulewise ? t2x * 8 : 0);
    w->tkey_s = take(modulewise ? t2x * 8 : 0);
    w->rowstart = take(modulewise ? ((size_t)N + 1) * 4 : 0);
    w->temp_bytes = t1 > t2 ? t1 : t2;
    w->temp = take(w->temp_bytes + 256);
    w->total = off;
    return HGNN_OK;
}

unsigned tp_grid(int64_t n) {
    const int64_t b = ceil_div(n > 0 ? n : 1, kBlock);
    return (unsigned)(b < kTpMaxBlocks ? b : kTpMaxBlocks);
}

#define TP_FOR(i, n) \
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < (n); i += (int64_t)gridDim.x * kBlock)

// column c of [mte, mte.flip(0)]
__device__ __forceinline__ void tp_column(const int64_t* __restrict__ mte, int64_t T, int64_t c, int64_t& a,
                                          int64_t& b) {
    const int64_t e = c < T ? c : c - T;
    const int64_t x = mte[e], y = mte[T + e];
    a = c < T ? x : y;
    b = c < T ? y : x;
}

// flag[c] = column c belongs to e_bidir (always 0 in the pid mode, where key == NULL: that part is empty there)
__global__ __launch_bounds__(kBlock) void k_tp_truth(const int64_t* __restrict__ mte, int64_t T, int64_t N,
                                                     const uint8_t* __restrict__ sm, uint64_t* __restrict__ key,
                                                     int32_t* __restrict__ flag, int32_t* __restrict__ status) {
    bool bad = false;
    TP_FOR(c, 2 * T) {
        int64_t a, b;
        tp_column(mte, T, c, a, b);
        bool keep = false;
        if (a < 0 || a >= N || b < 0 || b >= N) bad = true;
        else keep = key != nullptr && sm[a] != 0 && sm[b] != 0;
        flag[c] = keep ? 1 : 0;
        if (key != nullptr) key[c] = keep ? ((uint64_t)a << kTpIdBits) | (uint64_t)b : kTpNoKey;
    }
    if (bad) atomicOr(status, HGNN_TP_ST_BAD_MTE);
}

// rowstart[i], i in [0, N]: the first of the M sorted keys that is >= i << 31 (the sentinels sort behind row N - 1)
__global__ __launch_bounds__(kBlock) void k_tp_rowstart(const uint64_t* __restrict__ tkey, int64_t M, int64_t N,
                                                        int32_t* __restrict__ rowstart) {
    TP_FOR(i, N + 1) {
        const uint64_t k = (uint64_t)i << kTpIdBits;
        int64_t lo = 0, hi = M;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (tkey[mid] < k) lo = mid + 1;
            else hi = mid;
        }
        rowstart[i] = (int32_t)lo;
    }
}

struct TpRows {
    const int64_t* idx;
    int64_t N;
    int32_t K;
    const int64_t* pid;
    const uint8_t* sm;
    const uint64_t* tkey;        // sorted e_bidir keys (modulewise)
    const int32_t* rowstart;     // [N + 1] (modulewise)
};

// slot `slot` of a row: the id, or kTpNoId for an empty slot, a slot past K and a bad id
__device__ __forceinline__ int32_t tp_slot(const int64_t* __restrict__ row, int slot, int K, int64_t N, bool& bad) {
    if (slot >= K) return kTpNoId;
    const int64_t v = row[slot];
    if (v >= 0 && v < N) return (int32_t)v;
    if (v != -1) bad = true;
    return kTpNoId;
}

__device__ __forceinline__ int32_t tp_exchange(int32_t v, int j, bool keep_min) {
    const int32_t o = __shfl_xor(v, j, kWave);
    return keep_min ? (v < o ? v : o) : (v > o ? v : o);
}

// bitonic sort, ascending, of the 64 (a) or 128 (a, b) values of a wave; element e = h * 64 + lane with h = 0 for a
// and 1 for b.  Stage k, step j: e is compared with e ^ j and the pair is ascending iff (e & k) == 0.
template <bool TWO>
__device__ __forceinline__ void tp_sort(int32_t& a, int32_t& b, int lane) {
#pragma unroll
    for (int k = 2; k <= kWave; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j >= 1; j >>= 1) {
            const bool lower = (lane & j) == 0;
            const bool asc = k == kWave ? true : (lane & k) == 0;
            a = tp_exchange(a, j, lower == asc);
            if (TWO) b = tp_exchange(b, j, lower == (k == kWave ? false : asc));   // e & 64 is set in the b half
        }
    }
    if (TWO) {
        // stage 128, all ascending: step 64 pairs a with b inside the lane, the steps below it stay in their half
        const int32_t lo = a < b ? a : b, hi = a < b ? b : a;
        a = lo, b = hi;
#pragma unroll
        for (int j = kWave >> 1; j >= 1; j >>= 1) {
            const bool lower = (lane & j) == 0;
            a = tp_exchange(a, j, lower);
            b = tp_exchange(b, j, lower);
        }
    }
}

// whether row i emits the id v of one of its slots; modulewise: [rs, re) is the row's run of sorted e_bidir keys
template <bool MODULEWISE>
__device__ __forceinline__ bool tp_emit(const TpRows& r, int64_t i, int64_t pid_i, bool sm_i, int32_t rs, int32_t re,
                                        int32_t v, bool valid) {
    if (!valid) return false;
    const int64_t pid_v = r.pid[v];
    if (MODULEWISE) {
        if (!(pid_i != pid_v || pid_i == 0 || pid_v == 0)) return false;
        const uint64_t k = ((uint64_t)i << kTpIdBits) | (uint64_t)v;
        int32_t lo = rs, hi = re;
        while (lo < hi) {
            const int32_t mid = (lo + hi) >> 1;
            if (r.tkey[mid] < k) lo = mid + 1;
            else hi = mid;
        }
        return !(lo < re && r.tkey[lo] == k);
    }
    if (sm_i && r.sm[v] != 0) return false;
    return !(pid_i == pid_v && pid_i != 0 && pid_v != 0);
}

// one wave per row; FILL = false: counts[i]; FILL = true: the pairs at offs[i] + rank
template <bool MODULEWISE, bool TWO, bool FILL>
__global__ __launch_bounds__(kBlock) void k_tp_rows(TpRows r, int32_t* __restrict__ counts,
                                                    const int32_t* __restrict__ offs, int32_t* __restrict__ status,
                                                    int64_t* __restrict__ out_graph, uint8_t* __restrict__ out_y,
                                                    int64_t cap) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t first = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int64_t stride = (int64_t)gridDim.x * kWavesPerBlock;
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    bool bad = false;
    for (int64_t i = first; i < r.N; i += stride) {              // wave-uniform: all 64 lanes stay together
        const int64_t* row = r.idx + i * r.K;
        int32_t a = tp_slot(row, lane, r.K, r.N, bad);
        int32_t b = TWO ? tp_slot(row, lane + kWave, r.K, r.N, bad) : kTpNoId;
        bool va = a != kTpNoId, vb = TWO && b != kTpNoId;
        int32_t rs = 0, re = 0;
        if (MODULEWISE) {
            tp_sort<TWO>(a, b, lane);
            const int32_t pa = __shfl_up(a, 1, kWave);
            va = a != kTpNoId && (lane == 0 || a != pa);
            if (TWO) {
                const int32_t pb = __shfl_up(b, 1, kWave), last_a = __shfl(a, kWave - 1, kWave);
                vb = b != kTpNoId && b != (lane == 0 ? last_a : pb);
            }
            rs = r.rowstart[i], re = r.rowstart[i + 1];
        }
        const int64_t pid_i = r.pid[i];
        const bool sm_i = r.sm[i] != 0;
        const bool ea = tp_emit<MODULEWISE>(r, i, pid_i, sm_i, rs, re, a, va);
        const bool eb = TWO ? tp_emit<MODULEWISE>(r, i, pid_i, sm_i, rs, re, b, vb) : false;
        const uint64_t ma = __ballot(ea), mb = TWO ? __ballot(eb) : 0;
        const int na = __popcll(ma);
        if (!FILL) {
            if (lane == 0) counts[i] = na + __popcll(mb);
        } else {
            const int64_t base = offs[i];
            const int64_t p_a = base + __popcll(ma & below), p_b = base + na + __popcll(mb & below);
            if (ea && p_a < cap) {
                out_graph[p_a] = i;
                out_graph[cap + p_a] = a;
                out_y[p_a] = 0;
            }
            if (TWO && eb && p_b < cap) {
                out_graph[p_b] = i;
                out_graph[cap + p_b] = b;
                out_y[p_b] = 0;
            }
        }
    }
    if (!FILL && bad) atomicOr(status, HGNN_TP_ST_BAD_IDX);
}

__global__ void k_tp_info(const int32_t* __restrict__ counts, const int32_t* __restrict__ offs, int64_t N, int64_t L,
                          const int32_t* __restrict__ status, int64_t* __restrict__ info) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int64_t P = (int64_t)offs[L - 1] + counts[L - 1];
    const int64_t n_row = N < L ? (int64_t)offs[N] : P;
    info[HGNN_TP_P] = P;
    info[HGNN_TP_N_ROW] = n_row;
    info[HGNN_TP_N_TRUTH] = P - n_row;
    info[HGNN_TP_STATUS] = *status;
}

__global__ __launch_bounds__(kBlock) void k_tp_truth_fill(const int64_t* __restrict__ mte, int64_t T,
                                                          const int32_t* __restrict__ flag,
                                                          const int32_t* __restrict__ pos,
                                                          int64_t* __restrict__ out_graph,
                                                          uint8_t* __restrict__ out_y, int64_t cap) {
    TP_FOR(c, 2 * T) {
        if (flag[c] == 0) continue;
        const int64_t p = pos[c];
        if (p < 0 || p >= cap) continue;
        int64_t a, b;
        tp_column(mte, T, c, a, b);
        out_graph[p] = a;
        out_graph[cap + p] = b;
        out_y[p] = 1;
    }
}

template <bool FILL>
void tp_launch_rows(const TpRows& r, bool modulewise, int32_t* counts, const int32_t* offs, int32_t* status,
                    int64_t* out_graph, uint8_t* out_y, int64_t cap, hipStream_t stream) {
    const int64_t blocks = ceil_div(r.N, kWavesPerBlock);
    const unsigned grid = (unsigned)(blocks < kTpMaxBlocks ? blocks : kTpMaxBlocks);
    const bool two = r.K > kWave;
#define TP_ROWS(MW, TWO) \
    k_tp_rows<MW, TWO, FILL><<<grid, kBlock, 0, stream>>>(r, counts, offs, status, out_graph, out_y, cap)
    if (modulewise) {
        if (two) TP_ROWS(true, true);
        else TP_ROWS(true, false);
    } else {
        if (two) TP_ROWS(false, true);
        else TP_ROWS(false, false);
    }
#undef TP_ROWS
}

int tp_check(const char* who, int64_t N, int32_t K, int64_t T, int32_t mode) {
    HGNN_REQUIRE(N >= 0 && N <= kTpMaxN, "%s: n = %lld outside [0, 2^31)", who, (long long)N);
    HGNN_REQUIRE(K >= 1 && K <= HGNN_TP_MAX_K, "%s: K = %d outside [1, %d]", who, (int)K, HGNN_TP_MAX_K);
    HGNN_REQUIRE(T >= 0 && T <= kTpMaxN / 4, "%s: t = %lld outside [0, 2^29)", who, (long long)T);
    HGNN_REQUIRE(N * K + 2 * T <= kTpMaxN, "%s: n * K + 2 t = %lld pairs: positions are int32", who,
                 (long long)(N * K + 2 * T));
    HGNN_REQUIRE(mode == HGNN_TP_MODE_MODULEWISE || mode == HGNN_TP_MODE_PID, "%s: unknown mode %d", who, (int)mode);
    return HGNN_OK;
}

}  // namespace
}  // namespace hgnn

using namespace hgnn;

extern "C" int hgnn_training_pairs_workspace_bytes(int64_t n, int32_t K, int64_t t, int32_t mode, size_t* bytes) {
    const char* who = "hgnn_training_pairs_workspace_bytes";
    HGNN_REQUIRE(bytes != nullptr, "%s: bytes is NULL", who);
    int rc = tp_check(who, n, K, t, mode);
    if (rc != HGNN_OK) return rc;
    TpWorkspace w;
    rc = tp_layout(n, t, mode == HGNN_TP_MODE_MODULEWISE, &w, nullptr);
    if (rc != HGNN_OK) return rc;
    *bytes = w.total;
    return HGNN_OK;
}

extern "C" int hgnn_training_pairs_count(const int64_t* idx, int64_t n, int32_t K, const int64_t* mte, int64_t t,
                                         const uint8_t* signal_mask, const int64_t* pid, int32_t mode, int64_t* info,
                                         void* workspace, size_t workspace_bytes, hgnn_stream_t stream_) {
    const char* who = "hgnn_training_pairs_count";
    hipStream_t stream = (hipStream_t)stream_;
    int rc = tp_check(who, n, K, t, mode);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE(info != nullptr, "%s: info is NULL", who);
    HGNN_CHECK_HIP(hipMemsetAsync(info, 0, HGNN_TP_INFO * sizeof(int64_t), stream));
    if (n == 0 && t == 0) return HGNN_OK;
    HGNN_REQUIRE(n == 0 || (idx != nullptr && signal_mask != nullptr && pid != nullptr), "%s: NULL pointer", who);
    HGNN_REQUIRE(t == 0 || mte != nullptr, "%s: mte is NULL", who);
    const bool mw = mode == HGNN_TP_MODE_MODULEWISE;
    TpWorkspace w;
    rc = tp_layout(n, t, mw, &w, stream);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE_WORKSPACE(who, workspace, workspace_bytes, w.total);
    char* ws = (char*)workspace;
    int32_t *counts = (int32_t*)(ws + w.counts), *offs = (int32_t*)(ws + w.offs), *status = (int32_t*)(ws + w.status);
    uint64_t *tkey = mw ? (uint64_t*)(ws + w.tkey) : nullptr, *tkey_s = mw ? (uint64_t*)(ws + w.tkey_s) : nullptr;
    int32_t* rowstart = mw ? (int32_t*)(ws + w.rowstart) : nullptr;
    const int64_t L = n + 2 * t;
    size_t tb = w.temp_bytes;

    HGNN_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), stream));
    if (t > 0) {
        k_tp_truth<<<tp_grid(2 * t), kBlock, 0, stream>>>(mte, t, n, signal_mask, tkey, counts + n, status);
        if (mw)
            HGNN_CHECK_HIP(rocprim::radix_sort_keys(ws + w.temp, tb, tkey, tkey_s, (size_t)(2 * t), 0u, kTpKeyBits,
                                                    stream));
    }
    if (n > 0) {
        if (mw) k_tp_rowstart<<<tp_grid(n + 1), kBlock, 0, stream>>>(tkey_s, 2 * t, n, rowstart);
        const TpRows r{idx, n, K, pid, signal_mask, tkey_s, rowstart};
        tp_launch_rows<false>(r, mw, counts, nullptr, status, nullptr, nullptr, 0, stream);
    }
    tb = w.temp_bytes;
    HGNN_CHECK_HIP(rocprim::exclusive_scan(ws + w.temp, tb, counts, offs, (int32_t)0, (size_t)L,
                                           rocprim::plus<int32_t>(), stream));
    k_tp_info<<<1, kWave, 0, stream>>>(counts, offs, n, L, status, info);
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}

extern "C" int hgnn_training_pairs_fill(const int64_t* idx, int64_t n, int32_t K, const int64_t* mte, int64_t t,
                                        const uint8_t* signal_mask, const int64_t* pid, int32_t mode,
                                        int64_t* out_graph, uint8_t* out_y, int64_t cap, const void* workspace,
                                        size_t workspace_bytes, hgnn_stream_t stream_) {
    const char* who = "hgnn_training_pairs_fill";
    hipStream_t stream = (hipStream_t)stream_;
    int rc = tp_check(who, n, K, t, mode);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE(cap >= 0 && cap <= n * K + 2 * t, "%s: cap = %lld outside [0, n * K + 2 t]", who, (long long)cap);
    if (cap == 0 || (n == 0 && t == 0)) return HGNN_OK;
    HGNN_REQUIRE(out_graph != nullptr && out_y != nullptr, "%s: NULL output", who);
    HGNN_REQUIRE(n == 0 || (idx != nullptr && signal_mask != nullptr && pid != nullptr), "%s: NULL pointer", who);
    HGNN_REQUIRE(t == 0 || mte != nullptr, "%s: mte is NULL", who);
    const bool mw = mode == HGNN_TP_MODE_MODULEWISE;
    TpWorkspace w;
    rc = tp_layout(n, t, mw, &w, stream);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE_WORKSPACE(who, workspace, workspace_bytes, w.total);
    const char* ws = (const char*)workspace;
    const int32_t *counts = (const int32_t*)(ws + w.counts), *offs = (const int32_t*)(ws + w.offs);
    if (n > 0) {
        const TpRows r{idx, n, K, pid, signal_mask, mw ? (const uint64_t*)(ws + w.tkey_s) : nullptr,
                       mw ? (const int32_t*)(ws + w.rowstart) : nullptr};
        tp_launch_rows<true>(r, mw, nullptr, offs, nullptr, out_graph, out_y, cap, stream);
    }
    if (mw && t > 0)
        k_tp_truth_fill<<<tp_grid(2 * t), kBlock, 0, stream>>>(mte, t, counts + n, offs + n, out_graph, out_y, cap);
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}
