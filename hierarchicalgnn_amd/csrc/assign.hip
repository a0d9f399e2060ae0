// Max-weight bipartite matching of the assignment loss (reference BipartiteClassification/
// bipartite_classification_base.py:152-191 and gmrt_base.py:159-198; scipy CSR + min_weight_full_bipartite_matching
// on the host there).  DESIGN.md section 3, "Assignment loss", has the derivations.
//
// Contraction (the pattern of intersect.hip):
//   pack     key = row << 31 | col, ids checked against [0, n_rows) x [0, n_cols) (a bad id sets the status)
//   sort     rocprim::radix_sort_pairs (key, original position), stable -> rocprim::unique -> U distinct pairs
//   sum      per distinct pair the float64 sum of its scores in ascending original position (the only floating-point
//            sum; fixed order, so two calls give the same bits); q = rint(w * 2^S) * (n + 1), n = n_rows + n_cols
//
// Matching: a symmetric perfect assignment on the doubled graph, solved by an integer eps-scaled Jacobi auction.
//   persons  rows r in [0, P), cols' P + c          objects  cols c in [0, C), rows' C + r
//   edges    (r, c) and (c', r') with the pair's q; (r, r') with the fallback's q; (c', c) with 0
//   Both halves of an optimal perfect assignment are optimal matchings of the original problem; the row half is
//   returned.  With every q a multiple of n + 1 the assignment found at eps = 1 is exactly optimal for q.
//   A round: every unassigned person finds the best and second-best value a - price over its edges (one wave per
//   person, ties to the smallest object) and bids price + best - second + eps; every object takes the highest bid,
//   ties to the smallest person (a 64-bit atomicMax of the bid, then a 32-bit atomicMin of the person among those
//   that bid exactly the maximum: the two-step form keeps all 62 bits of the bid), and evicts its owner.
//   Between phases (eps -> eps / 8) an assignment is kept when it still satisfies eps-CS at the new eps.
//   Rounds with many bidders are three grid launches; the tails with few bidders run in ONE workgroup that keeps
//   the bidder list in LDS and loops until no bidder is left or its round budget is spent.  No grid-wide barrier
//   anywhere, every loop bounded.  The host reads {U, status, max |q|} once and then one state vector per tail
//   launch: at most kAmMaxReads reads, after which the call gives up with HGNN_AM_ST_BUDGET.
#include "common.h"
#include <climits>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>

namespace hgnn {
namespace {

using u64 = unsigned long long;

constexpr int kAmIdBits = 31;
constexpr unsigned kAmKeyBits = 2 * kAmIdBits;
constexpr uint64_t kAmIdMask = ((uint64_t)1 << kAmIdBits) - 1;
constexpr int64_t kAmQMax = (int64_t)1 << 56;       // |q| limit
constexpr int64_t kAmBig = (int64_t)1 << 57;        // bid increment of a person with a single edge
constexpr int64_t kAmPriceMax = (int64_t)1 << 61;   // a price or an increment above this: HGNN_AM_ST_OVERFLOW
constexpr int64_t kAmNeg = INT64_MIN;
constexpr int kAmTailThreads = 1024, kAmTailWaves = kAmTailThreads / kWave;
constexpr int kAmTailCap = 1024;       // bidders one tail launch accepts (LDS lists)
constexpr int kAmTailBudget = 16384;   // rounds of one tail launch
constexpr int kAmFat0 = 8, kAmFatMax = 256;   // grid rounds in front of a tail launch; doubled when the tail declines
constexpr int kAmMaxReads = 48;        // host reads of one call (the loss around it adds 6; 64 is documented)

// device state vector (int64)
enum { AM_U = 0, AM_STATUS, AM_QMAX, AM_UNASSIGNED, AM_ROUNDS, AM_NEED_GRID, AM_STATE };

#define AM_LD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define AM_ST(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

struct AmGraph {
    int32_t P, C;
    const int32_t *rp, *radj, *cp, *cadj;   // row-major and column-major CSR of the distinct pairs
    const int64_t *rq, *cq;
    int64_t qf;                             // fallback edge
};

struct AmVars {
    int64_t* price;    // [n] objects
    u64* bidmax;       // [n] highest bid seen by an object (== price once the round is over)
    int32_t* winner;   // [n] INT_MAX between rounds
    int32_t* owner;    // [n] object -> person, -1
    int32_t* pobj;     // [n] person -> object, -1
    int32_t* pbj;      // [n] grid rounds: the object a person bids for, -1 = no bid
    int64_t* pbid;     // [n] grid rounds: its bid
    int64_t* st;       // [AM_STATE]
};

struct AmWorkspace {
    size_t key, key_s, pos, pos_s, ukey, count, rq, radj, cq, cadj, rp, cp, price, bidmax, pbid, winner, owner, pobj,
        pbj, st, temp, temp_bytes, total;
};

int am_layout(int64_t B, int64_t P, int64_t C, AmWorkspace* w, hipStream_t stream) {
    size_t t1 = 0, t2 = 0;
    HGNN_CHECK_HIP(rocprim::radix_sort_pairs(nullptr, t1, (uint64_t*)nullptr, (uint64_t*)nullptr, (int32_t*)nullptr,
                                             (int32_t*)nullptr, (size_t)B, 0u, kAmKeyBits, stream));
    HGNN_CHECK_HIP(rocprim::unique(nullptr, t2, (uint64_t*)nullptr, (uint64_t*)nullptr, (size_t*)nullptr, (size_t)B,
                                   rocprim::equal_to<uint64_t>(), stream));
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    };
    const size_t b = (size_t)B, n = (size_t)(P + C);
    w->key = take(b * 8);
    w->key_s = take(b * 8);
    w->pos = take(b * 4);
    w->pos_s = take(b * 4);
    w->ukey = take(b * 8);
    w->count = take(sizeof(size_t));
    w->rq = take(b * 8);
    w->radj = take(b * 4);
    w->cq = take(b * 8);
    w->cadj = take(b * 4);
    w->rp = take(((size_t)P + 1) * 4);
    w->cp = take(((size_t)C + 1) * 4);
    w->price = take(n * 8);
    w->bidmax = take(n * 8);
    w->pbid = take(n * 8);
    w->winner = take(n * 4);
    w->owner = take(n * 4);
    w->pobj = take(n * 4);
    w->pbj = take(n * 4);
    w->st = take(AM_STATE * 8);
    w->temp_bytes = t1 > t2 ? t1 : t2;
    w->temp = take(w->temp_bytes + 256);
    w->total = off;
    return HGNN_OK;
}

unsigned am_blocks(int64_t n) { return (unsigned)ceil_div(n > 0 ? n : 1, 256); }

__global__ __launch_bounds__(256) void k_am_pack(const int64_t* __restrict__ row, const int64_t* __restrict__ col,
                                                 int64_t B, int64_t P, int64_t C, uint64_t* __restrict__ key,
                                                 int32_t* __restrict__ pos, int64_t* __restrict__ st) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    int64_t r = row[i], c = col[i];
    if (r < 0 || r >= P || c < 0 || c >= C) {
        atomicOr((u64*)&st[AM_STATUS], (u64)HGNN_AM_ST_BAD_ID);
        r = c = 0;
    }
    key[i] = ((uint64_t)r << kAmIdBits) | (uint64_t)c;
    pos[i] = (int32_t)i;
}

// one thread per distinct pair: the float64 sum of its scores in original order, its quantised weight, and the
// (col, row) key of the column-major sort
__global__ __launch_bounds__(256) void k_am_contract(const uint64_t* __restrict__ ukey,
                                                     const size_t* __restrict__ count,
                                                     const uint64_t* __restrict__ key_s,
                                                     const int32_t* __restrict__ pos_s, int64_t B,
                                                     const float* __restrict__ score, int64_t n1,
                                                     int64_t* __restrict__ pair_row, int64_t* __restrict__ pair_col,
                                                     double* __restrict__ pair_w, int64_t* __restrict__ rq,
                                                     int32_t* __restrict__ radj, uint64_t* __restrict__ ckey,
                                                     int32_t* __restrict__ cidx, int64_t* __restrict__ st) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t U = (int64_t)*count;
    if (i == 0) st[AM_U] = U;
    if (i >= U) return;
    const uint64_t k = ukey[i];
    int64_t lo = 0, hi = B;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (key_s[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    double s = 0;
    for (int64_t j = lo; j < B && key_s[j] == k; ++j) s += (double)score[pos_s[j]];
    const int64_t r = (int64_t)(k >> kAmIdBits), c = (int64_t)(k & kAmIdMask);
    pair_row[i] = r;
    pair_col[i] = c;
    pair_w[i] = s;
    const double x = rint(s * (double)((int64_t)1 << HGNN_AM_SCALE_BITS));
    int64_t q = 0;
    if (!(fabs(x) <= (double)(kAmQMax / n1))) atomicOr((u64*)&st[AM_STATUS], (u64)HGNN_AM_ST_BAD_WEIGHT);  // NaN too
    else q = (int64_t)x * n1;
    rq[i] = q;
    radj[i] = (int32_t)c;
    atomicMax((u64*)&st[AM_QMAX], (u64)(q < 0 ? -q : q));
    ckey[i] = ((uint64_t)c << kAmIdBits) | (uint64_t)r;
    cidx[i] = (int32_t)i;
}

__device__ inline int32_t am_lower(const uint64_t* __restrict__ a, int64_t n, uint64_t k) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return (int32_t)lo;
}

// CSR pointers of both orders and the initial auction state
__global__ __launch_bounds__(256) void k_am_setup(const uint64_t* __restrict__ ukey, const uint64_t* __restrict__ ckey_s,
                                                  int64_t U, int32_t P, int32_t C, int32_t* __restrict__ rp,
                                                  int32_t* __restrict__ cp, AmVars s) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i <= P) rp[i] = am_lower(ukey, U, (uint64_t)i << kAmIdBits);
    if (i <= C) cp[i] = am_lower(ckey_s, U, (uint64_t)i << kAmIdBits);
    if (i < (int64_t)P + C) {
        s.price[i] = 0;
        s.bidmax[i] = 0;
        s.pbid[i] = 0;
        s.winner[i] = INT_MAX;
        s.owner[i] = -1;
        s.pobj[i] = -1;
        s.pbj[i] = -1;
    }
}

__global__ __launch_bounds__(256) void k_am_cadj(const uint64_t* __restrict__ ckey_s, const int32_t* __restrict__ cidx_s,
                                                 int64_t U, const int64_t* __restrict__ rq, int32_t* __restrict__ cadj,
                                                 int64_t* __restrict__ cq) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= U) return;
    cadj[i] = (int32_t)(ckey_s[i] & kAmIdMask);
    cq[i] = rq[cidx_s[i]];
}

// ---- the auction -------------------------------------------------------------------------------------------------

struct AmBest {
    int64_t v1, v2, p1;   // best and second-best value, price of the best object
    int32_t j1;
};

__device__ inline int am_degree(const AmGraph& g, int32_t i) {
    return 1 + (i < g.P ? g.rp[i + 1] - g.rp[i] : g.cp[i - g.P + 1] - g.cp[i - g.P]);
}

// edge t of person i: t == 0 is the implicit edge (r, r') or (c', c)
__device__ inline void am_edge(const AmGraph& g, int32_t i, int t, int32_t* obj, int64_t* a) {
    if (i < g.P) {
        if (t == 0) {
            *obj = g.C + i;
            *a = g.qf;
        } else {
            const int32_t e = g.rp[i] + t - 1;
            *obj = g.radj[e];
            *a = g.rq[e];
        }
    } else {
        const int32_t c = i - g.P;
        if (t == 0) {
            *obj = c;
            *a = 0;
        } else {
            const int32_t e = g.cp[c] + t - 1;
            *obj = g.C + g.cadj[e];
            *a = g.cq[e];
        }
    }
}

// One wave scans person i: every lane returns the best / second-best value over all of i's edges (ties of the best to
// the smallest object).  With `held` >= 0, *vheld receives the value of that object.
__device__ inline AmBest am_scan(const AmGraph& g, const int64_t* price, int32_t i, int lane, int32_t held,
                                 int64_t* vheld) {
    AmBest b{kAmNeg, kAmNeg, 0, INT_MAX};
    int64_t vh = kAmNeg;
    const int deg = am_degree(g, i);
    for (int t = lane; t < deg; t += kWave) {
        int32_t j;
        int64_t a;
        am_edge(g, i, t, &j, &a);
        const int64_t p = AM_LD(&price[j]);
        const int64_t v = a - p;
        if (j == held) vh = v;
        if (v > b.v1 || (v == b.v1 && j < b.j1)) {
            b.v2 = b.v1;
            b.v1 = v;
            b.j1 = j;
            b.p1 = p;
        } else if (v > b.v2) {
            b.v2 = v;
        }
    }
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) {
        const int64_t ov1 = __shfl_xor((long long)b.v1, m, kWave), ov2 = __shfl_xor((long long)b.v2, m, kWave);
        const int64_t op1 = __shfl_xor((long long)b.p1, m, kWave);
        const int32_t oj1 = __shfl_xor(b.j1, m, kWave);
        const int64_t ovh = __shfl_xor((long long)vh, m, kWave);
        if (ov1 > b.v1 || (ov1 == b.v1 && oj1 < b.j1)) {
            b.v2 = b.v1 > ov2 ? b.v1 : ov2;
            b.v1 = ov1;
            b.j1 = oj1;
            b.p1 = op1;
        } else {
            b.v2 = b.v2 > ov1 ? b.v2 : ov1;
        }
        vh = vh > ovh ? vh : ovh;
    }
    if (vheld != nullptr) *vheld = vh;
    return b;
}

// the bid of a scan; false = it would leave the int64 range this kernel guards
__device__ inline bool am_bid(const AmBest& b, int64_t eps, int64_t* bid) {
    const int64_t inc = b.v2 == kAmNeg ? kAmBig : b.v1 - b.v2;
    if (b.p1 > kAmPriceMax || inc > kAmPriceMax) return false;
    *bid = b.p1 + inc + eps;
    return true;
}

// grid round, step 1: one wave per person
__global__ __launch_bounds__(256) void k_am_bid(AmGraph g, AmVars s, int64_t eps) {
    const int32_t n = g.P + g.C;
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) / kWave;
    const int lane = threadIdx.x & (kWave - 1);
    if (i >= n) return;
    if (s.pobj[i] >= 0) {
        if (lane == 0) s.pbj[i] = -1;
        return;
    }
    const AmBest b = am_scan(g, s.price, (int32_t)i, lane, -1, nullptr);
    if (lane != 0) return;
    int64_t bid;
    if (!am_bid(b, eps, &bid)) {
        atomicOr((u64*)&s.st[AM_STATUS], (u64)HGNN_AM_ST_OVERFLOW);
        s.pbj[i] = -1;
        return;
    }
    s.pbj[i] = b.j1;
    s.pbid[i] = bid;
    atomicMax(&s.bidmax[b.j1], (u64)bid);
}

// step 2: among the persons that bid an object's maximum, the smallest
__global__ __launch_bounds__(256) void k_am_win(int32_t n, AmVars s) {
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t j = s.pbj[i];
    if (j >= 0 && (u64)s.pbid[i] == s.bidmax[j]) atomicMin(&s.winner[j], i);
}

// step 3: the winner takes the object (only it touches owner / price / winner of that object)
__global__ __launch_bounds__(256) void k_am_assign(int32_t n, AmVars s) {
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t j = s.pbj[i];
    if (j < 0 || AM_LD(&s.winner[j]) != i) return;
    const int32_t old = s.owner[j];
    s.owner[j] = i;
    s.price[j] = s.pbid[i];
    s.pobj[i] = j;
    AM_ST(&s.winner[j], INT_MAX);
    if (old >= 0) s.pobj[old] = -1;
}

// phase start: drop the assignments that break eps-CS at the new eps
__global__ __launch_bounds__(256) void k_am_recheck(AmGraph g, AmVars s, int64_t eps) {
    const int32_t n = g.P + g.C;
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) / kWave;
    const int lane = threadIdx.x & (kWave - 1);
    if (i >= n) return;
    const int32_t j = s.pobj[i];
    if (j < 0) return;
    int64_t vh;
    const AmBest b = am_scan(g, s.price, (int32_t)i, lane, j, &vh);
    if (lane == 0 && vh < b.v1 - eps) {
        s.owner[j] = -1;
        s.pobj[i] = -1;
    }
}

// The tail: ONE workgroup runs rounds until no bidder is left, `budget` rounds are spent or a bid overflows.  The
// bidder list lives in LDS; a launch that finds more than kAmTailCap bidders declines (AM_NEED_GRID) and the host
// runs more grid rounds.  Every word another wave of this workgroup wrote in global memory is read with an
// agent-scope load or an atomic (served by L2), so a copy in this CU's L1 is never trusted.
__global__ __launch_bounds__(kAmTailThreads) void k_am_tail(AmGraph g, AmVars s, int64_t eps, int budget) {
    __shared__ int32_t list[2][kAmTailCap];
    __shared__ int32_t sbj[kAmTailCap];
    __shared__ int64_t sbid[kAmTailCap];
    __shared__ int cnt[2];
    __shared__ int bad;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int32_t n = g.P + g.C;
    if (tid == 0) {
        cnt[0] = cnt[1] = 0;
        bad = 0;
    }
    __syncthreads();
    for (int32_t i = tid; i < n; i += kAmTailThreads)
        if (s.pobj[i] < 0) {
            const int k = atomicAdd(&cnt[0], 1);
            if (k < kAmTailCap) list[0][k] = i;
        }
    __syncthreads();
    int m = cnt[0];
    if (m > kAmTailCap) {
        if (tid == 0) {
            s.st[AM_UNASSIGNED] = m;
            s.st[AM_NEED_GRID] = 1;
        }
        return;
    }
    int cur = 0, rounds = 0;
    while (m > 0 && rounds < budget) {
        for (int k = wave; k < m; k += kAmTailWaves) {
            const AmBest b = am_scan(g, s.price, list[cur][k], lane, -1, nullptr);
            if (lane == 0) {
                int64_t bid = 0;
                if (am_bid(b, eps, &bid)) atomicMax(&s.bidmax[b.j1], (u64)bid);
                else bad = 1;
                sbj[k] = b.j1;
                sbid[k] = bid;
            }
        }
        if (tid == 0) cnt[cur ^ 1] = 0;
        __syncthreads();
        if (bad) break;
        for (int k = tid; k < m; k += kAmTailThreads) {
            const int32_t j = sbj[k];
            if ((u64)sbid[k] == AM_LD(&s.bidmax[j])) atomicMin(&s.winner[j], list[cur][k]);
        }
        __syncthreads();
        for (int k = tid; k < m; k += kAmTailThreads) {
            const int32_t j = sbj[k];
            if (AM_LD(&s.winner[j]) == list[cur][k]) sbj[k] = ~j;   // negative: this bidder won
        }
        __syncthreads();
        for (int k = tid; k < m; k += kAmTailThreads) {
            const int32_t i = list[cur][k];
            int32_t j = sbj[k];
            int32_t next = i;
            if (j < 0) {
                j = ~j;
                next = AM_LD(&s.owner[j]);
                AM_ST(&s.owner[j], i);
                AM_ST(&s.price[j], sbid[k]);
                AM_ST(&s.pobj[i], j);
                AM_ST(&s.winner[j], INT_MAX);
                if (next >= 0) AM_ST(&s.pobj[next], -1);
            }
            if (next >= 0) list[cur ^ 1][atomicAdd(&cnt[cur ^ 1], 1)] = next;   // never more than m entries
        }
        __syncthreads();
        cur ^= 1;
        m = cnt[cur];
        ++rounds;
    }
    if (tid == 0) {
        if (bad) atomicOr((u64*)&s.st[AM_STATUS], (u64)HGNN_AM_ST_OVERFLOW);
        s.st[AM_UNASSIGNED] = m;
        s.st[AM_ROUNDS] += rounds;
        s.st[AM_NEED_GRID] = 0;
    }
}

__global__ __launch_bounds__(256) void k_am_emit(int32_t P, int32_t C, const int32_t* __restrict__ pobj,
                                                 int64_t* __restrict__ col_match) {
    const int32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= P) return;
    const int32_t j = pobj[r];
    col_match[r] = (j >= 0 && j < C) ? (int64_t)j : (int64_t)C + r;
}

}  // namespace
}  // namespace hgnn

using namespace hgnn;

static int am_check(const char* who, int64_t B, int64_t P, int64_t C) {
    HGNN_REQUIRE(B > 0 && P > 0 && C > 0, "%s: n_edges, n_rows and n_cols must be positive", who);
    HGNN_REQUIRE(B < ((int64_t)1 << 31) - 1, "%s: more than 2^31 - 2 edges", who);
    HGNN_REQUIRE(P + C < ((int64_t)1 << 30), "%s: n_rows + n_cols must stay below 2^30", who);
    return HGNN_OK;
}

extern "C" int hgnn_assign_match_workspace_bytes(int64_t n_edges, int64_t n_rows, int64_t n_cols, size_t* bytes) {
    int rc = am_check("hgnn_assign_match_workspace_bytes", n_edges, n_rows, n_cols);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE(bytes != nullptr, "hgnn_assign_match_workspace_bytes: NULL bytes");
    AmWorkspace w;
    rc = am_layout(n_edges, n_rows, n_cols, &w, nullptr);
    if (rc != HGNN_OK) return rc;
    *bytes = w.total;
    return HGNN_OK;
}

extern "C" int hgnn_assign_match(const int64_t* row, const int64_t* col, const float* score, int64_t n_edges,
                                 int64_t n_rows, int64_t n_cols, int64_t* col_match, int64_t* pair_row,
                                 int64_t* pair_col, double* pair_weight, int64_t* info, void* workspace,
                                 size_t workspace_bytes, hgnn_stream_t stream_) {
    const char* who = "hgnn_assign_match";
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t B = n_edges, P = n_rows, C = n_cols, n = n_rows + n_cols;
    int rc = am_check(who, B, P, C);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE(row != nullptr && col != nullptr && score != nullptr, "%s: NULL input", who);
    HGNN_REQUIRE(col_match != nullptr && pair_row != nullptr && pair_col != nullptr && pair_weight != nullptr &&
                     info != nullptr,
                 "%s: NULL output", who);
    AmWorkspace w;
    rc = am_layout(B, P, C, &w, stream);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE_WORKSPACE(who, workspace, workspace_bytes, w.total);
    char* ws = (char*)workspace;
    uint64_t *key = (uint64_t*)(ws + w.key), *key_s = (uint64_t*)(ws + w.key_s), *ukey = (uint64_t*)(ws + w.ukey);
    int32_t *pos = (int32_t*)(ws + w.pos), *pos_s = (int32_t*)(ws + w.pos_s);
    size_t* count = (size_t*)(ws + w.count);
    int64_t *rq = (int64_t*)(ws + w.rq), *cq = (int64_t*)(ws + w.cq);
    int32_t *radj = (int32_t*)(ws + w.radj), *cadj = (int32_t*)(ws + w.cadj);
    int32_t *rp = (int32_t*)(ws + w.rp), *cp = (int32_t*)(ws + w.cp);
    void* temp = ws + w.temp;
    size_t tb = w.temp_bytes;
    AmVars s;
    s.price = (int64_t*)(ws + w.price);
    s.bidmax = (u64*)(ws + w.bidmax);
    s.pbid = (int64_t*)(ws + w.pbid);
    s.winner = (int32_t*)(ws + w.winner);
    s.owner = (int32_t*)(ws + w.owner);
    s.pobj = (int32_t*)(ws + w.pobj);
    s.pbj = (int32_t*)(ws + w.pbj);
    s.st = (int64_t*)(ws + w.st);
    for (int k = 0; k < HGNN_AM_INFO; ++k) info[k] = 0;

    // contraction
    HGNN_CHECK_HIP(hipMemsetAsync(s.st, 0, AM_STATE * 8, stream));
    k_am_pack<<<am_blocks(B), 256, 0, stream>>>(row, col, B, P, C, key, pos, s.st);
    HGNN_CHECK_HIP(rocprim::radix_sort_pairs(temp, tb, key, key_s, pos, pos_s, (size_t)B, 0u, kAmKeyBits, stream));
    HGNN_CHECK_HIP(rocprim::unique(temp, tb, key_s, ukey, count, (size_t)B, rocprim::equal_to<uint64_t>(), stream));
    // key / pos are free from here on: they take the (col, row) keys of the column-major order
    k_am_contract<<<am_blocks(B), 256, 0, stream>>>(ukey, count, key_s, pos_s, B, score, n + 1, pair_row, pair_col,
                                                    pair_weight, rq, radj, key, pos, s.st);
    HGNN_CHECK_HIP(hipGetLastError());
    int64_t st[AM_STATE];
    int64_t reads = 0;
    auto read_state = [&]() -> hipError_t {
        ++reads;
        hipError_t e = hipMemcpyAsync(st, s.st, sizeof(st), hipMemcpyDeviceToHost, stream);
        return e != hipSuccess ? e : hipStreamSynchronize(stream);
    };
    HGNN_CHECK_HIP(read_state());
    const int64_t U = st[AM_U];
    info[HGNN_AM_N_PAIRS] = U;
    info[HGNN_AM_HOST_READS] = reads;
    if (st[AM_STATUS] != 0) {
        info[HGNN_AM_STATUS] = st[AM_STATUS];
        return HGNN_OK;
    }

    // both CSR orders
    HGNN_CHECK_HIP(rocprim::radix_sort_pairs(temp, tb, key, key_s, pos, pos_s, (size_t)U, 0u, kAmKeyBits, stream));
    const int64_t m1 = (P > C ? P : C) + 1;
    k_am_setup<<<am_blocks(m1 > n ? m1 : n), 256, 0, stream>>>(ukey, key_s, U, (int32_t)P, (int32_t)C, rp, cp, s);
    k_am_cadj<<<am_blocks(U), 256, 0, stream>>>(key_s, pos_s, U, rq, cadj, cq);
    AmGraph g;
    g.P = (int32_t)P;
    g.C = (int32_t)C;
    g.rp = rp;
    g.radj = radj;
    g.cp = cp;
    g.cadj = cadj;
    g.rq = rq;
    g.cq = cq;
    g.qf = (int64_t)rint(HGNN_AM_FALLBACK_WEIGHT * (double)((int64_t)1 << HGNN_AM_SCALE_BITS)) * (n + 1);

    const unsigned wave_blocks = am_blocks(n * kWave), blocks = am_blocks(n);
    int64_t eps = st[AM_QMAX] / 4 > 1 ? st[AM_QMAX] / 4 : 1;
    int64_t phases = 0, grid_rounds = 0, status = 0;
    for (;;) {
        ++phases;
        if (phases > 1) k_am_recheck<<<wave_blocks, 256, 0, stream>>>(g, s, eps);
        int fat = kAmFat0;
        for (;;) {
            for (int f = 0; f < fat; ++f) {
                k_am_bid<<<wave_blocks, 256, 0, stream>>>(g, s, eps);
                k_am_win<<<blocks, 256, 0, stream>>>((int32_t)n, s);
                k_am_assign<<<blocks, 256, 0, stream>>>((int32_t)n, s);
            }
            grid_rounds += fat;
            k_am_tail<<<1, kAmTailThreads, 0, stream>>>(g, s, eps, kAmTailBudget);
            HGNN_CHECK_HIP(hipGetLastError());
            HGNN_CHECK_HIP(read_state());
            status = st[AM_STATUS];
            if (status != 0 || st[AM_UNASSIGNED] == 0) break;
            if (reads >= kAmMaxReads) {
                status = HGNN_AM_ST_BUDGET;
                break;
            }
            if (st[AM_NEED_GRID] != 0 && fat < kAmFatMax) fat *= 2;
        }
        if (status != 0 || eps == 1) break;
        eps = eps / 8 > 1 ? eps / 8 : 1;
    }
    if (status == 0) k_am_emit<<<am_blocks(P), 256, 0, stream>>>((int32_t)P, (int32_t)C, s.pobj, col_match);
    HGNN_CHECK_HIP(hipGetLastError());
    info[HGNN_AM_STATUS] = status;
    info[HGNN_AM_PHASES] = phases;
    info[HGNN_AM_GRID_ROUNDS] = grid_rounds;
    info[HGNN_AM_TAIL_ROUNDS] = st[AM_ROUNDS];
    info[HGNN_AM_HOST_READS] = reads;
    return HGNN_OK;
}
