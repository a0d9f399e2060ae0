// Per-particle and per-candidate tracking records with binned counts: hgnn_track_records.
//
// The pipeline is hgnn_track_eval's (trackeval.hip; the kernels and the workspace layout are shared through
// trackeval_common.h): the same sorts, contingency triples, match rule and fixed-order reduction, so result[] has
// the same bits.  What the scalar entry folds into 12 doubles is kept here:
//
//   candidates  after the dense relabel, one thread per run writes label / size of the kept candidates and clears
//               their counters
//   matching    k_te_match<true>: per particle (one wave, no atomics) the smallest kept candidate index, that
//               triple's n and the hits in masked triples; per candidate integer atomicAdd (kept, masked) and a
//               64-bit atomicMin of p << 32 | n over its kept matches.  The triples are row-major by particle, so
//               the candidate side is the scattered one; integer atomics give the same result in any order
//   tables      per particle (one wave): pt and every binning variable reduced over the particle's hits (the
//               minimum in which a NaN wins and -0.0 is below 0.0), and the fields copied out of the workspace;
//               per candidate the packed minimum is split into (particle, shared)
//   histogram   one thread per particle and variable: slot = number of float32 edges <= value (a NaN goes to the
//               overflow slot), six integer columns per slot in per-block LDS counters, flushed with 64-bit
//               integer atomics on vector memory
//
// No float atomics, as in trackeval.hip; every count is an integer, so two calls give the same bits.
#include "trackeval_common.h"

#pragma clang fp contract(off)

namespace hgnn {
namespace {

constexpr int kMaxVars = HGNN_TR_MAX_VARS;
constexpr int kSlots = HGNN_TR_MAX_BINS + 2;
constexpr int kCols = HGNN_TR_COLUMNS;
constexpr int kHistBlocks = 256;

struct TrBins {  // by value in the kernel arguments: the caller's edges are host memory
    float edges[kMaxVars][HGNN_TR_MAX_BINS + 1];
    int32_t nb[kMaxVars];
};

struct TrWorkspace {
    TeWorkspace te;
    size_t c_first, masked_hits, total;
};

int tr_layout(int64_t B, int64_t N, TrWorkspace* w, hipStream_t stream) {
    int rc = te_layout(B, N, &w->te, stream);
    if (rc != HGNN_OK) return rc;
    size_t off = w->te.total;
    w->c_first = off;
    off = align_up(off + (size_t)B * 8, 256);
    w->masked_hits = off;
    off = align_up(off + (size_t)N * 4, 256);
    w->total = off;
    return HGNN_OK;
}

// label, size and cleared counters of every kept candidate (run r of the label-sorted pairs -> dense index c)
__global__ __launch_bounds__(256) void k_tr_cand_table(const int64_t* __restrict__ ck,
                                                       const int32_t* __restrict__ cstart,
                                                       const int32_t* __restrict__ crid,
                                                       const int32_t* __restrict__ keep,
                                                       const int32_t* __restrict__ kscan, int B,
                                                       hgnn_tr_candidates t, unsigned long long* __restrict__ c_first) {
    int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= B || r >= crid[B - 1] || keep[r] == 0) return;
    const int c = kscan[r] - 1;
    t.label[c] = ck[cstart[r]];
    t.size[c] = cstart[r + 1] - cstart[r];
    t.n_kept[c] = 0;
    t.n_mask[c] = 0;
    c_first[c] = ~0ull;
}

__global__ __launch_bounds__(256) void k_tr_cand_final(const unsigned long long* __restrict__ c_first,
                                                       const int32_t* __restrict__ kscan, int B,
                                                       hgnn_tr_candidates t) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= B || c >= kscan[B - 1]) return;
    const unsigned long long f = c_first[c];
    const bool any = f != ~0ull;
    t.particle[c] = any ? (int32_t)(f >> 32) : -1;
    t.shared[c] = any ? (int32_t)(f & 0xffffffffu) : 0;
}

// no pairs: no triple, so no match; the particles are still there and reconstructable or not
__global__ __launch_bounds__(256) void k_tr_no_pairs(const int32_t* __restrict__ prid, int N,
                                                     const int32_t* __restrict__ nhits,
                                                     const float* __restrict__ ptmin,
                                                     const int32_t* __restrict__ prim, TeParams prm,
                                                     int4* __restrict__ pp_cnt, int32_t* __restrict__ cand_index,
                                                     int32_t* __restrict__ shared, int32_t* __restrict__ masked_hits) {
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= N || p >= prid[N - 1]) return;
    const bool prim_ok = !prm.use_primary || prim[p] != 0;
    const bool recon = ptmin[p] > prm.pt_cut && (double)nhits[p] >= prm.nhits_cut && prim_ok;
    pp_cnt[p] = make_int4(0, 0, 0, recon ? 1 : 0);
    cand_index[p] = -1;
    shared[p] = 0;
    masked_hits[p] = 0;
}

// The table's minimum: nan_min made independent of the order of the hits.  Equal floats differ in bits only as
// -0.0 and 0.0; the negative zero wins (the minimum of the total order), so the stored bits are defined.  The pipeline's
// ptmin (k_te_particles) is only ever compared, where the sign of a zero does not show; the table's pt is reduced here
__device__ inline float table_min(float m, float v) {
    return (v < m || v != v || (v == m && __float_as_uint(v) > __float_as_uint(m))) ? v : m;
}

__device__ inline float wave_table_min(const float* __restrict__ x, const int32_t* __restrict__ pv, int b, int e,
                                       int lane) {
    float m = __builtin_inff();
    for (int j = b + lane; j < e; j += 64) m = table_min(m, x[pv[j]]);
    for (int o = 32; o > 0; o >>= 1) m = table_min(m, __shfl_xor(m, o));
    return m;
}

// one wave per particle: pt and the binning variables over its hits, and the fields the pipeline left in the workspace
__global__ __launch_bounds__(256) void k_tr_particle_table(const int32_t* __restrict__ pstart,
                                                           const int32_t* __restrict__ prid,
                                                           const int32_t* __restrict__ pv, int N,
                                                           const float* __restrict__ pt,
                                                           const float* __restrict__ vars, int n_vars,
                                                           const int32_t* __restrict__ nhits,
                                                           const int64_t* __restrict__ opid,
                                                           const int32_t* __restrict__ prim,
                                                           const int4* __restrict__ pp_cnt, hgnn_tr_particles t) {
    const int lane = threadIdx.x & 63;
    const int P = prid[N - 1];
    for (int p = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; p < P; p += (gridDim.x * blockDim.x) >> 6) {
        const int b = pstart[p], e = pstart[p + 1];
        for (int v = 0; v < n_vars; ++v) {
            const float m = wave_table_min(vars + (size_t)v * N, pv, b, e, lane);
            if (lane == 0) t.values[(size_t)v * N + p] = m;
        }
        const float ptm = wave_table_min(pt, pv, b, e, lane);
        if (lane == 0) {
            const int4 c = pp_cnt[p];
            t.pid[p] = opid[p];
            t.nhits[p] = nhits[p];
            t.pt[p] = ptm;
            t.primary[p] = prim[p] != 0;
            t.reconstructable[p] = c.w != 0;
            t.n_match[p] = c.x;
            t.n_kept[p] = c.y;
            t.n_mask[p] = c.z;
        }
    }
}

// slot of x among nb + 1 ascending edges: the number of edges <= x (numpy.searchsorted(edges, x, "right")); numpy
// orders a NaN after every number, so it lands in the overflow slot nb + 1
__device__ inline int slot_of(const float* edges, int nb, float x) {
    if (x != x) return nb + 1;
    int s = 0;
    for (int k = 0; k <= nb; ++k) s += edges[k] <= x;
    return s;
}

__global__ __launch_bounds__(256) void k_tr_hist(const int32_t* __restrict__ prid, int N, int n_vars, TrBins bins,
                                                 const float* __restrict__ values, const int4* __restrict__ pp_cnt,
                                                 const int32_t* __restrict__ nhits,
                                                 const int32_t* __restrict__ masked_hits,
                                                 unsigned long long* __restrict__ hist) {
    __shared__ unsigned long long s_h[kMaxVars * kSlots * kCols];
    __shared__ float s_e[kMaxVars][HGNN_TR_MAX_BINS + 1];
    __shared__ int s_nb[kMaxVars];
    const int tid = threadIdx.x;
    const int cells = n_vars * kSlots * kCols;
    for (int i = tid; i < cells; i += 256) s_h[i] = 0;
    for (int i = tid; i < n_vars * (HGNN_TR_MAX_BINS + 1); i += 256)
        s_e[i / (HGNN_TR_MAX_BINS + 1)][i % (HGNN_TR_MAX_BINS + 1)] =
            bins.edges[i / (HGNN_TR_MAX_BINS + 1)][i % (HGNN_TR_MAX_BINS + 1)];
    if (tid < n_vars) s_nb[tid] = bins.nb[tid];
    __syncthreads();
    const int P = prid[N - 1];
    for (int p = blockIdx.x * 256 + tid; p < P; p += gridDim.x * 256) {
        const int4 c = pp_cnt[p];
        const unsigned long long nh = (unsigned long long)nhits[p], mh = (unsigned long long)masked_hits[p];
        for (int v = 0; v < n_vars; ++v) {
            const int slot = slot_of(s_e[v], s_nb[v], values[(size_t)v * N + p]);
            unsigned long long* h = s_h + (v * kSlots + slot) * kCols;
            atomicAdd(h + 0, 1ull);
            if (c.w != 0) atomicAdd(h + 1, 1ull);
            if (c.y != 0) atomicAdd(h + 2, (unsigned long long)c.y);
            if (c.z != 0) {
                atomicAdd(h + 3, (unsigned long long)c.z);
                atomicAdd(h + 4, mh);
                atomicAdd(h + 5, nh * (unsigned long long)c.z);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < cells; i += 256)
        if (s_h[i] != 0) atomicAdd(hist + i, s_h[i]);
}

unsigned hist_blocks(int64_t n) {
    int64_t b = ceil_div(n > 0 ? n : 1, 256);
    return (unsigned)(b < kHistBlocks ? b : kHistBlocks);
}

}  // namespace
}  // namespace hgnn

using namespace hgnn;

static int tr_check_vars(const char* who, int32_t n_vars) {
    HGNN_REQUIRE(n_vars >= 0 && n_vars <= kMaxVars, "%s: n_vars %d outside [0, %d]", who, (int)n_vars, kMaxVars);
    return HGNN_OK;
}

extern "C" int hgnn_track_records_workspace_bytes(int64_t n_pairs, int64_t n_hits, int32_t n_vars, size_t* bytes) {
    int rc = te_check_sizes("hgnn_track_records_workspace_bytes", n_pairs, n_hits);
    if (rc != HGNN_OK) return rc;
    rc = tr_check_vars("hgnn_track_records_workspace_bytes", n_vars);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE(bytes != nullptr, "hgnn_track_records_workspace_bytes: NULL bytes");
    TrWorkspace w;
    rc = tr_layout(n_pairs, n_hits, &w, nullptr);
    if (rc != HGNN_OK) return rc;
    *bytes = w.total;
    return HGNN_OK;
}

extern "C" int hgnn_track_records(const int64_t* hit, const int64_t* cand, int64_t n_pairs, const int64_t* pid,
                                  const float* pt, const uint8_t* primary, int64_t n_hits, const float* vars,
                                  int32_t n_vars, const float* edges, const int32_t* n_bins, double pt_cut,
                                  double nhits_cut, double majority_cut, double* result,
                                  const hgnn_tr_particles* particles, const hgnn_tr_candidates* candidates,
                                  int64_t* hist, void* workspace, size_t workspace_bytes, hgnn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char* who = "hgnn_track_records";
    int rc = te_check_sizes(who, n_pairs, n_hits);
    if (rc != HGNN_OK) return rc;
    rc = tr_check_vars(who, n_vars);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE(result != nullptr, "%s: NULL result", who);
    HGNN_REQUIRE(majority_cut > 0.0, "%s: majority_cut must be > 0", who);
    HGNN_REQUIRE(n_pairs == 0 || (hit != nullptr && cand != nullptr), "%s: NULL pair arrays", who);
    HGNN_REQUIRE(n_hits == 0 || (pid != nullptr && pt != nullptr), "%s: NULL event arrays", who);
    HGNN_REQUIRE(n_pairs == 0 || n_hits > 0, "%s: %lld pairs but no hits", who, (long long)n_pairs);
    hgnn_tr_particles pt_tab{};
    hgnn_tr_candidates c_tab{};
    if (n_hits > 0) {
        HGNN_REQUIRE(particles != nullptr, "%s: NULL particle table", who);
        pt_tab = *particles;
        HGNN_REQUIRE(pt_tab.pid && pt_tab.nhits && pt_tab.pt && pt_tab.primary && pt_tab.reconstructable &&
                         pt_tab.n_match && pt_tab.n_kept && pt_tab.n_mask && pt_tab.cand_index && pt_tab.shared,
                     "%s: NULL particle table column", who);
        HGNN_REQUIRE(n_vars == 0 || (vars != nullptr && pt_tab.values != nullptr),
                     "%s: NULL vars or particle values with n_vars > 0", who);
    }
    if (n_pairs > 0) {
        HGNN_REQUIRE(candidates != nullptr, "%s: NULL candidate table", who);
        c_tab = *candidates;
        HGNN_REQUIRE(c_tab.label && c_tab.size && c_tab.n_kept && c_tab.n_mask && c_tab.particle && c_tab.shared,
                     "%s: NULL candidate table column", who);
    }
    TrBins bins{};
    if (n_vars > 0) {
        HGNN_REQUIRE(edges != nullptr && n_bins != nullptr && hist != nullptr, "%s: NULL edges, n_bins or hist", who);
        for (int v = 0; v < n_vars; ++v) {
            const int nb = n_bins[v];
            HGNN_REQUIRE(nb >= 1 && nb <= HGNN_TR_MAX_BINS, "%s: n_bins[%d] = %d outside [1, %d]", who, v, nb,
                         HGNN_TR_MAX_BINS);
            const float* e = edges + (size_t)v * (HGNN_TR_MAX_BINS + 1);
            for (int k = 0; k <= nb; ++k) {
                HGNN_REQUIRE(e[k] - e[k] == 0.0f, "%s: edge %d of variable %d is not finite", who, k, v);
                HGNN_REQUIRE(k == 0 || e[k - 1] < e[k], "%s: edges of variable %d are not strictly ascending", who, v);
                bins.edges[v][k] = e[k];
            }
            bins.nb[v] = nb;
        }
    }
    TrWorkspace w;
    rc = tr_layout(n_pairs, n_hits, &w, stream);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE_WORKSPACE(who, workspace, workspace_bytes, w.total);
    char* ws = (char*)workspace;
    auto I32 = [&](size_t o) { return (int32_t*)(ws + o); };
    const int B = (int)n_pairs, N = (int)n_hits;
    const int cbits = bit_width(B), pbits = bit_width(N);
    void* temp = ws + w.te.temp;
    size_t tb = w.te.temp_bytes;
    const TeWorkspace& te = w.te;

    int32_t *pv_in = I32(te.pv_in), *pv = I32(te.pv), *pflag = I32(te.pflag), *prid = I32(te.prid);
    int32_t *pstart = I32(te.pstart), *hit_p = I32(te.hit_p), *nhits = I32(te.nhits), *prim = I32(te.prim);
    int32_t* masked_hits = I32(w.masked_hits);
    int64_t *pk = (int64_t*)(ws + te.pk), *opid = (int64_t*)(ws + te.opid);
    float* ptmin = (float*)(ws + te.ptmin);
    int4* pp_cnt = (int4*)(ws + te.pp_cnt);
    TeParams prm{majority_cut, nhits_cut, majority_cut * nhits_cut, (float)pt_cut, primary != nullptr ? 1 : 0};

    if (n_vars > 0)
        HGNN_CHECK_HIP(hipMemsetAsync(hist, 0, (size_t)n_vars * kSlots * kCols * sizeof(int64_t), stream));

    if (N > 0) {  // step 2 first: the particles do not depend on the pairs
        k_te_iota<<<blocks_for(N), 256, 0, stream>>>(pv_in, N);
        HGNN_CHECK_HIP(rocprim::radix_sort_pairs(temp, tb, pid, pk, pv_in, pv, (size_t)N, 0u, 64u, stream));
        k_te_heads<int64_t, false><<<blocks_for(N), 256, 0, stream>>>(pk, N, 0, pflag);
        HGNN_CHECK_HIP(rocprim::inclusive_scan(temp, tb, pflag, prid, (size_t)N, rocprim::plus<int32_t>(), stream));
        k_te_starts<int64_t, false><<<blocks_for(N), 256, 0, stream>>>(pk, pflag, prid, N, 0, pstart);
        k_te_hit_particle<<<blocks_for(N), 256, 0, stream>>>(pv, prid, N, hit_p);
        k_te_particles<<<wave_blocks(N), 256, 0, stream>>>(pstart, prid, pv, pk, pt, primary, N, nhits, opid, ptmin,
                                                           prim);
    }
    if (B > 0) {
        int32_t *cv_in = I32(te.cv_in), *cv = I32(te.cv), *cflag = I32(te.cflag), *crid = I32(te.crid);
        int32_t *cstart = I32(te.cstart), *ckeep = I32(te.ckeep), *kscan = I32(te.kscan), *ccol = I32(te.ccol);
        int64_t* ck = (int64_t*)(ws + te.ck);
        uint64_t *key = (uint64_t*)(ws + te.key), *skey = (uint64_t*)(ws + te.skey);
        int32_t *tflag = I32(te.tflag), *trid = I32(te.trid), *tstart = I32(te.tstart);
        int32_t *prow_b = I32(te.prow_b), *prow_e = I32(te.prow_e), *err = I32(te.err);
        double* pp_sum = (double*)(ws + te.pp_sum);
        unsigned long long* c_first = (unsigned long long*)(ws + w.c_first);
        const uint64_t sentinel = (uint64_t)N << cbits;

        HGNN_CHECK_HIP(hipMemsetAsync(err, 0, sizeof(int32_t), stream));
        HGNN_CHECK_HIP(hipMemsetAsync(prow_b, 0, (size_t)N * 4, stream));
        HGNN_CHECK_HIP(hipMemsetAsync(prow_e, 0, (size_t)N * 4, stream));

        // step 1: candidate runs, size filter, dense relabel; the candidate table's label and size
        k_te_iota<<<blocks_for(B), 256, 0, stream>>>(cv_in, B);
        HGNN_CHECK_HIP(rocprim::radix_sort_pairs(temp, tb, cand, ck, cv_in, cv, (size_t)B, 0u, 64u, stream));
        k_te_heads<int64_t, false><<<blocks_for(B), 256, 0, stream>>>(ck, B, 0, cflag);
        HGNN_CHECK_HIP(rocprim::inclusive_scan(temp, tb, cflag, crid, (size_t)B, rocprim::plus<int32_t>(), stream));
        k_te_starts<int64_t, false><<<blocks_for(B), 256, 0, stream>>>(ck, cflag, crid, B, 0, cstart);
        const float thr = (float)(nhits_cut * majority_cut);
        k_te_cand_keep<<<blocks_for(B), 256, 0, stream>>>(cstart, crid, B, thr, ckeep);
        HGNN_CHECK_HIP(rocprim::inclusive_scan(temp, tb, ckeep, kscan, (size_t)B, rocprim::plus<int32_t>(), stream));
        k_tr_cand_table<<<blocks_for(B), 256, 0, stream>>>(ck, cstart, crid, ckeep, kscan, B, c_tab, c_first);

        // step 3: contingency triples (p, c, n), row-major
        k_te_pair_keys<<<blocks_for(B), 256, 0, stream>>>(cv, crid, cstart, ckeep, kscan, hit, hit_p, B, N, cbits,
                                                          key, ccol, err);
        HGNN_CHECK_HIP(rocprim::radix_sort_keys(temp, tb, key, skey, (size_t)B, 0u, (unsigned)(pbits + cbits),
                                                stream));
        k_te_heads<uint64_t, true><<<blocks_for(B), 256, 0, stream>>>(skey, B, sentinel, tflag);
        HGNN_CHECK_HIP(rocprim::inclusive_scan(temp, tb, tflag, trid, (size_t)B, rocprim::plus<int32_t>(), stream));
        k_te_starts<uint64_t, true><<<blocks_for(B), 256, 0, stream>>>(skey, tflag, trid, B, sentinel, tstart);
        k_te_rows<<<blocks_for(B), 256, 0, stream>>>(skey, tstart, trid, B, cbits, prow_b, prow_e);

        // steps 4-7, keeping the records
        TeMatchRecords<true> rec{pt_tab.cand_index, pt_tab.shared, masked_hits, c_tab.n_kept, c_tab.n_mask, c_first};
        k_te_match<true><<<wave_blocks(N), 256, 0, stream>>>(prow_b, prow_e, skey, tstart, ccol, kscan, prid, nhits,
                                                             opid, ptmin, prim, B, N, cbits, prm, pp_sum, pp_cnt, rec);
        k_tr_cand_final<<<blocks_for(B), 256, 0, stream>>>(c_first, kscan, B, c_tab);
        k_te_reduce<<<kRedBlocks, 256, 0, stream>>>(pp_sum, pp_cnt, prid, N, (double*)(ws + te.blk_sum),
                                                    (long long*)(ws + te.blk_cnt));
        k_te_finalize<<<1, kRedBlocks, 0, stream>>>((double*)(ws + te.blk_sum), (long long*)(ws + te.blk_cnt), prid,
                                                    kscan, B, N, err, result);
    } else {
        // no pairs: hgnn_track_eval's default response; the particle table and the particle columns are still filled
        if (N > 0)
            k_tr_no_pairs<<<blocks_for(N), 256, 0, stream>>>(prid, N, nhits, ptmin, prim, prm, pp_cnt,
                                                             pt_tab.cand_index, pt_tab.shared, masked_hits);
        k_te_finalize<<<1, kRedBlocks, 0, stream>>>(nullptr, nullptr, prid, nullptr, 0, N, nullptr, result);
    }
    if (N > 0) {
        k_tr_particle_table<<<wave_blocks(N), 256, 0, stream>>>(pstart, prid, pv, N, pt, vars, n_vars, nhits, opid,
                                                                prim, pp_cnt, pt_tab);
        if (n_vars > 0)
            k_tr_hist<<<hist_blocks(N), 256, 0, stream>>>(prid, N, n_vars, bins, pt_tab.values, pp_cnt, nhits,
                                                          masked_hits, (unsigned long long*)hist);
    }
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}
