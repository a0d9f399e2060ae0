// Tracking-performance metrics of a hit -> track-candidate assignment (reference
// Modules/tracking_utils.py:18-83, eval_metrics; cupy / cupy.sparse there).
//
// Every step stays on the device; the caller reads back only the small result
// vector.  Data flow (B = pairs, N = hits; every array is in the workspace):
//
//   candidates  sort (cand, pair) by cand [rocprim::radix_sort_pairs, 64 bits, B]
//               -> run heads -> inclusive scan = run id -> run starts
//               -> keep run iff float(count) >= float(nhits_cut * majority_cut)
//               -> inclusive scan of keep = dense label c (ascending label order), C
//   particles   sort (pid, hit) by pid [rocprim::radix_sort_pairs, 64 bits, N]
//               -> heads / scan / starts as above = particle p (ascending pid), P
//               -> per particle (one wave): nhits, original pid, min pt, any primary
//               -> hit_p[hit] = p
//   contingency key(pair) = p << cbits | c (filtered pairs: sentinel N << cbits)
//               sorted [rocprim::radix_sort_keys, bits 0 .. pbits + cbits, B]
//               -> runs of equal keys = triples (p, c, n) in row-major order,
//               col[c] = the candidate's run length, row ranges of every particle
//   matching    per particle (one wave): row max of n * h_c, then the three
//               match conditions, the match filter and the masks of every triple;
//               per-particle partial counts and sums
//   result      fixed-order two-level reduction over particles (256 blocks, then
//               one block) -> the metrics, written to result[HGNN_TE_*]
//
// rocPRIM calls: radix_sort_pairs<int64, int32> (twice), radix_sort_keys<uint64>,
// inclusive_scan<int32, plus> (four times).  They share one temporary region,
// sized by the largest query; the stream orders them.
//
// Numerics.  Counts are integers (no float atomics anywhere; the only atomic
// is the error flag).  Everything after the contingency table is fp64; the
// hash h_c restates numpy's linspace(1, 1 + 1e-12, C) without contraction
// (the pragma below; HIP's __dmul_rn / __dadd_rn are header inlines that hipcc
// still fuses into v_fma_f64).
// The two means are sums in a fixed order (lanes, wave butterfly, blocks of
// particles, one final block), so two calls give the same bits.
//
// The kernels and the workspace layout are in trackeval_common.h, shared with
// hgnn_track_records (trackeval_records.hip), which runs the same pipeline and
// keeps the per-particle and per-candidate results.  This file instantiates
// k_te_match<false>: no store beyond the per-particle sums and counts.
#include "trackeval_common.h"

#pragma clang fp contract(off)

using namespace hgnn;

extern "C" int hgnn_track_eval_workspace_bytes(int64_t n_pairs, int64_t n_hits, size_t* bytes) {
    int rc = te_check_sizes("hgnn_track_eval_workspace_bytes", n_pairs, n_hits);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE(bytes != nullptr, "hgnn_track_eval_workspace_bytes: NULL bytes");
    TeWorkspace w;
    rc = te_layout(n_pairs, n_hits, &w, nullptr);
    if (rc != HGNN_OK) return rc;
    *bytes = w.total;
    return HGNN_OK;
}

extern "C" int hgnn_track_eval(const int64_t* hit, const int64_t* cand, int64_t n_pairs, const int64_t* pid,
                               const float* pt, const uint8_t* primary, int64_t n_hits, double pt_cut,
                               double nhits_cut, double majority_cut, double* result, void* workspace,
                               size_t workspace_bytes, hgnn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = te_check_sizes("hgnn_track_eval", n_pairs, n_hits);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE(result != nullptr, "hgnn_track_eval: NULL result");
    HGNN_REQUIRE(majority_cut > 0.0, "hgnn_track_eval: majority_cut must be > 0");
    HGNN_REQUIRE(n_pairs == 0 || (hit != nullptr && cand != nullptr), "hgnn_track_eval: NULL pair arrays");
    HGNN_REQUIRE(n_hits == 0 || (pid != nullptr && pt != nullptr), "hgnn_track_eval: NULL event arrays");
    HGNN_REQUIRE(n_pairs == 0 || n_hits > 0, "hgnn_track_eval: %lld pairs but no hits", (long long)n_pairs);
    TeWorkspace w;
    rc = te_layout(n_pairs, n_hits, &w, stream);
    if (rc != HGNN_OK) return rc;
    HGNN_REQUIRE_WORKSPACE("hgnn_track_eval", workspace, workspace_bytes, w.total);
    char* ws = (char*)workspace;
    auto I32 = [&](size_t o) { return (int32_t*)(ws + o); };
    const int B = (int)n_pairs, N = (int)n_hits;
    const int cbits = bit_width(B), pbits = bit_width(N);
    void* temp = ws + w.temp;
    size_t tb = w.temp_bytes;

    if (B > 0) {
        int32_t *cv_in = I32(w.cv_in), *cv = I32(w.cv), *cflag = I32(w.cflag), *crid = I32(w.crid);
        int32_t *cstart = I32(w.cstart), *ckeep = I32(w.ckeep), *kscan = I32(w.kscan), *ccol = I32(w.ccol);
        int64_t* ck = (int64_t*)(ws + w.ck);
        uint64_t *key = (uint64_t*)(ws + w.key), *skey = (uint64_t*)(ws + w.skey);
        int32_t *tflag = I32(w.tflag), *trid = I32(w.trid), *tstart = I32(w.tstart);
        int32_t *pv_in = I32(w.pv_in), *pv = I32(w.pv), *pflag = I32(w.pflag), *prid = I32(w.prid);
        int32_t *pstart = I32(w.pstart), *hit_p = I32(w.hit_p), *nhits = I32(w.nhits), *prim = I32(w.prim);
        int32_t *prow_b = I32(w.prow_b), *prow_e = I32(w.prow_e), *err = I32(w.err);
        int64_t *pk = (int64_t*)(ws + w.pk), *opid = (int64_t*)(ws + w.opid);
        float* ptmin = (float*)(ws + w.ptmin);
        double* pp_sum = (double*)(ws + w.pp_sum);
        int4* pp_cnt = (int4*)(ws + w.pp_cnt);
        const uint64_t sentinel = (uint64_t)N << cbits;

        HGNN_CHECK_HIP(hipMemsetAsync(err, 0, sizeof(int32_t), stream));
        HGNN_CHECK_HIP(hipMemsetAsync(prow_b, 0, (size_t)N * 4, stream));
        HGNN_CHECK_HIP(hipMemsetAsync(prow_e, 0, (size_t)N * 4, stream));

        // step 1: candidate runs, size filter, dense relabel
        k_te_iota<<<blocks_for(B), 256, 0, stream>>>(cv_in, B);
        HGNN_CHECK_HIP(rocprim::radix_sort_pairs(temp, tb, cand, ck, cv_in, cv, (size_t)B, 0u, 64u, stream));
        k_te_heads<int64_t, false><<<blocks_for(B), 256, 0, stream>>>(ck, B, 0, cflag);
        HGNN_CHECK_HIP(rocprim::inclusive_scan(temp, tb, cflag, crid, (size_t)B, rocprim::plus<int32_t>(), stream));
        k_te_starts<int64_t, false><<<blocks_for(B), 256, 0, stream>>>(ck, cflag, crid, B, 0, cstart);
        const float thr = (float)(nhits_cut * majority_cut);
        k_te_cand_keep<<<blocks_for(B), 256, 0, stream>>>(cstart, crid, B, thr, ckeep);
        HGNN_CHECK_HIP(rocprim::inclusive_scan(temp, tb, ckeep, kscan, (size_t)B, rocprim::plus<int32_t>(), stream));

        // step 2: particles
        k_te_iota<<<blocks_for(N), 256, 0, stream>>>(pv_in, N);
        HGNN_CHECK_HIP(rocprim::radix_sort_pairs(temp, tb, pid, pk, pv_in, pv, (size_t)N, 0u, 64u, stream));
        k_te_heads<int64_t, false><<<blocks_for(N), 256, 0, stream>>>(pk, N, 0, pflag);
        HGNN_CHECK_HIP(rocprim::inclusive_scan(temp, tb, pflag, prid, (size_t)N, rocprim::plus<int32_t>(), stream));
        k_te_starts<int64_t, false><<<blocks_for(N), 256, 0, stream>>>(pk, pflag, prid, N, 0, pstart);
        k_te_hit_particle<<<blocks_for(N), 256, 0, stream>>>(pv, prid, N, hit_p);
        k_te_particles<<<wave_blocks(N), 256, 0, stream>>>(pstart, prid, pv, pk, pt, primary, N, nhits, opid, ptmin,
                                                           prim);

        // step 3: contingency triples (p, c, n), row-major
        k_te_pair_keys<<<blocks_for(B), 256, 0, stream>>>(cv, crid, cstart, ckeep, kscan, hit, hit_p, B, N, cbits,
                                                          key, ccol, err);
        HGNN_CHECK_HIP(rocprim::radix_sort_keys(temp, tb, key, skey, (size_t)B, 0u, (unsigned)(pbits + cbits),
                                                stream));
        k_te_heads<uint64_t, true><<<blocks_for(B), 256, 0, stream>>>(skey, B, sentinel, tflag);
        HGNN_CHECK_HIP(rocprim::inclusive_scan(temp, tb, tflag, trid, (size_t)B, rocprim::plus<int32_t>(), stream));
        k_te_starts<uint64_t, true><<<blocks_for(B), 256, 0, stream>>>(skey, tflag, trid, B, sentinel, tstart);
        k_te_rows<<<blocks_for(B), 256, 0, stream>>>(skey, tstart, trid, B, cbits, prow_b, prow_e);

        // steps 4-7
        TeParams prm{majority_cut, nhits_cut, majority_cut * nhits_cut, (float)pt_cut, primary != nullptr ? 1 : 0};
        k_te_match<false><<<wave_blocks(N), 256, 0, stream>>>(prow_b, prow_e, skey, tstart, ccol, kscan, prid, nhits,
                                                              opid, ptmin, prim, B, N, cbits, prm, pp_sum, pp_cnt,
                                                              TeMatchRecords<false>{});
        k_te_reduce<<<kRedBlocks, 256, 0, stream>>>(pp_sum, pp_cnt, prid, N, (double*)(ws + w.blk_sum),
                                                    (long long*)(ws + w.blk_cnt));
        k_te_finalize<<<1, kRedBlocks, 0, stream>>>((double*)(ws + w.blk_sum), (long long*)(ws + w.blk_cnt), prid,
                                                    kscan, B, N, err, result);
    } else {
        // no pairs: default response; P is still counted when the event has hits
        int32_t *pv_in = I32(w.pv_in), *pv = I32(w.pv), *pflag = I32(w.pflag), *prid = I32(w.prid);
        int64_t* pk = (int64_t*)(ws + w.pk);
        if (N > 0) {
            k_te_iota<<<blocks_for(N), 256, 0, stream>>>(pv_in, N);
            HGNN_CHECK_HIP(rocprim::radix_sort_pairs(temp, tb, pid, pk, pv_in, pv, (size_t)N, 0u, 64u, stream));
            k_te_heads<int64_t, false><<<blocks_for(N), 256, 0, stream>>>(pk, N, 0, pflag);
            HGNN_CHECK_HIP(rocprim::inclusive_scan(temp, tb, pflag, prid, (size_t)N, rocprim::plus<int32_t>(),
                                                   stream));
        }
        k_te_finalize<<<1, kRedBlocks, 0, stream>>>(nullptr, nullptr, prid, nullptr, 0, N, nullptr, result);
    }
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}
