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
// The kernels, the workspace layout and the launch sequence (in stages) are in
// trackeval_common.h, shared with hgnn_track_scan (trackscan.hip), which runs the
// particle stage once for many pair sets of one event, and with
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
    const TePtrs p = te_ptrs(workspace, w);
    const int B = (int)n_pairs, N = (int)n_hits;
    size_t tb = p.temp_bytes;

    if (B > 0) {
        rc = te_clear(p, N, stream);
        if (rc != HGNN_OK) return rc;
        // step 1: candidate runs, size filter, dense relabel
        rc = te_candidate_runs(p, cand, B, stream);
        if (rc != HGNN_OK) return rc;
        const float thr = (float)(nhits_cut * majority_cut);
        k_te_cand_keep<<<blocks_for(B), 256, 0, stream>>>(p.cstart, p.crid, B, thr, p.ckeep);
        rc = te_candidate_relabel(p, B, stream);
        if (rc != HGNN_OK) return rc;
        // step 2: particles
        rc = te_particle_stage(p, pid, pt, primary, N, stream);
        if (rc != HGNN_OK) return rc;
        // step 3: contingency triples (p, c, n), row-major; steps 4-7
        TeParams prm{majority_cut, nhits_cut, majority_cut * nhits_cut, (float)pt_cut, primary != nullptr ? 1 : 0};
        rc = te_match_stage(p, hit, B, N, prm, stream);
        if (rc != HGNN_OK) return rc;
        k_te_finalize<<<1, kRedBlocks, 0, stream>>>(p.blk_sum, p.blk_cnt, p.prid, p.kscan, B, N, p.err, result);
    } else {
        // no pairs: default response; P is still counted when the event has hits
        if (N > 0) {
            k_te_iota<<<blocks_for(N), 256, 0, stream>>>(p.pv_in, N);
            HGNN_CHECK_HIP(rocprim::radix_sort_pairs(p.temp, tb, pid, p.pk, p.pv_in, p.pv, (size_t)N, 0u, 64u,
                                                     stream));
            k_te_heads<int64_t, false><<<blocks_for(N), 256, 0, stream>>>(p.pk, N, 0, p.pflag);
            HGNN_CHECK_HIP(rocprim::inclusive_scan(p.temp, tb, p.pflag, p.prid, (size_t)N, rocprim::plus<int32_t>(),
                                                   stream));
        }
        k_te_finalize<<<1, kRedBlocks, 0, stream>>>(nullptr, nullptr, p.prid, nullptr, 0, N, nullptr, result);
    }
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}
