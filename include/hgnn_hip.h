/*
 * hgnn_hip.h -- C ABI of libhgnn_hip.so: the MI355X (gfx950) message-passing
 * engine behind the reference's operator interface.
 *
 * Every entry point takes plain device pointers, sizes and a hipStream_t (as
 * void*), launches asynchronously on that stream, performs no allocation and no
 * host synchronisation (graph-capturable), and returns an int status
 * (HGNN_OK == 0).  hgnn_last_error() returns a thread-local message for the
 * last non-zero status.  No torch types appear here: a binding only needs
 * `tensor.data_ptr()` and the current stream handle.
 *
 * Reference interfaces these replace (paths relative to the reference root,
 * clairesonglee/HierarchicalGNN):
 *
 *   hgnn_plan_build / hgnn_segment_reduce_f32
 *       torch_scatter.scatter_add(src, index, dim=0, dim_size=N) as called at
 *       Modules/gnn_utils.py:50 and :125 (edge -> node aggregation, "K1"),
 *       Modules/gnn_utils.py:143 (weighted superedge -> supernode, "K4"),
 *       and, with a gather index, the fused expressions
 *       scatter_add(w * X[g], d, dim_size) at Modules/gnn_utils.py:124 ("K2"),
 *       :142 ("K3") and, with a per-row L1 scale,
 *       BipartiteClassification/Models/HGNN_GMM.py:269 ("K5").
 *   hgnn_spread_rows_f32
 *       backward of scatter_add (grad_src[e] = grad_out[index[e]]) and the gathers
 *       nodes[graph[0]], nodes[graph[1]] (Modules/gnn_utils.py:61) in destination order.
 *   hgnn_gather_rows_f32
 *       the row gathers nodes[graph[0]], nodes[graph[1]] at
 *       Modules/gnn_utils.py:61,134,152 ("K6"); also the backward of scatter_add.
 *   hgnn_edge_dot_f32
 *       backward of the weighted forms w.r.t. the weights (autograd of
 *       Modules/gnn_utils.py:124,142,143).
 *   hgnn_mlp_forward_f32
 *       the make_mlp Sequential (Modules/utils.py:169-196) of the edge / node networks
 *       fused with the concat + gathers feeding it and the skip connection
 *       (Modules/gnn_utils.py:52-53, :61-62): see the section at the end.
 */
#ifndef HGNN_HIP_H
#define HGNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HGNN_OK 0
#define HGNN_ERR_INVALID_ARG 1
#define HGNN_ERR_HIP 2
#define HGNN_ERR_WORKSPACE 3
#define HGNN_ERR_UNSUPPORTED 4

/* hgnn_assign_match and hgnn_assign_match_workspace_bytes were added without a bump: they are additions, and
 * no existing entry point, struct or constant changed layout or meaning.  The same holds for
 * hgnn_segment_reduce_f32_ex, hgnn_plan_item_order(_workspace_bytes), hgnn_get_option and the optimiser step
 * (hgnn_optim_*, hgnn_sizeof_opt_entry, struct hgnn_opt_entry, HGNN_OPT_*), for hgnn_wgrad_f32(_workspace_bytes) and for
 * hgnn_track_records(_workspace_bytes) with struct hgnn_tr_particles, struct hgnn_tr_candidates and HGNN_TR_*, and
 * for hgnn_training_pairs_workspace_bytes, hgnn_training_pairs_count and hgnn_training_pairs_fill with HGNN_TP_*, and
 * for hgnn_track_scan(_workspace_bytes) with HGNN_TS_*. */
#define HGNN_ABI_VERSION 26

typedef void* hgnn_stream_t; /* hipStream_t */

/* indices into hgnn_plan.counts (device int32[8]) */
#define HGNN_CNT_WORK 0     /* number of work items                         */
#define HGNN_CNT_SPLIT 1    /* number of destinations whose list was split  */
#define HGNN_CNT_PARTIAL 2  /* number of partial rows                       */
#define HGNN_CNT_ERR 3      /* !=0: an index was out of range (row dropped) */
#define HGNN_CNT_VALID 4    /* rows with a valid destination (and source)   */
#define HGNN_CNT_UNSORTED 5 /* !=0: the index was not already sorted by destination */

/*
 * A destination-sorted aggregation plan for one (index, dim_size) pair.  Built
 * once per event, reused by every cell (the topology is constant across the
 * 14 / 6+6 iterations of a forward: EdgeClassifier/Models/IN.py:87-88,
 * BipartiteClassification/Models/HGNN_GMM.py:93-94,:275-284).  All arrays are
 * device int32, allocated by the caller with the sizes hgnn_plan_dims() gives.
 */
typedef struct hgnn_plan {
    int64_t n_rows;    /* M: rows of `index` (edges)                              */
    int64_t n_dst;     /* N: dim_size                                             */
    int64_t n_src;     /* R: rows of the source table (== M when no gather index) */
    int32_t chunk;     /* longest list one wave sums; longer lists are split      */
    int32_t has_gather;
    int64_t max_work;     /* capacity of wi_*                                     */
    int64_t max_split;    /* capacity of split_dst; split_pbegin has +1           */
    int64_t max_partial;  /* rows of the partial-sum workspace                    */
    int32_t* perm;        /* [M]  original position of the p-th dst-sorted row (stable) */
    int32_t* src_row;     /* [M]  source-table row read at sorted position p; the caller may set it
                           *      to NULL when counts[HGNN_CNT_UNSORTED]==0 (index already sorted,
                           *      no gather): the reduce then streams rows p = begin..end contiguously */
    int32_t* dst32;       /* [M]  destination of ORIGINAL position e, -1 if invalid */
    int32_t* rowptr;      /* [N+1] CSR by destination over sorted positions       */
    int32_t* wi_begin;    /* [max_work]                                           */
    int32_t* wi_end;      /* [max_work]                                           */
    int32_t* wi_target;   /* [max_work] >=0: output row; <0: ~partial row         */
    int32_t* wi_dst;      /* [max_work] destination of the item (also for chunks) */
    int32_t* split_dst;   /* [max_split]                                          */
    int32_t* split_pbegin;/* [max_split+1] partial-row range of each split dst    */
    int32_t* counts;      /* [8]                                                  */
} hgnn_plan;

int hgnn_abi_version(void);
const char* hgnn_last_error(void);

/* sizeof(hgnn_plan) / sizeof(hgnn_mlp_desc) as compiled: lets a foreign-language binding
 * verify its struct mirror. */
int hgnn_sizeof_plan(void);
int hgnn_sizeof_mlp_desc(void);

/* Process-wide switches (diagnostics / A-B measurements).  NOT THREAD-SAFE: plain static ints read at launch time;
 * set them from the thread that launches, before the launches they should affect, never concurrently with one.
 * The defaults are the measured-best variants; everything a round measured slower has been removed from the library
 * (tools/experimental/ keeps the sources of the larger null results, DESIGN.md appendix A the numbers).
 *   "nt_loads"     1 (default): non-temporal loads of once-read source rows in K1..K5
 *   "nt_stores"    0 (default): non-temporal stores of gathered rows (K6)
 *   "mlp_split_variant" schedule of the feature-split bf16 MLP: -1 (default) per shape, 0 counted per-fragment
 *                  waits, 2 one wait per k-chunk ("burst")
 *   "mlp_ablate"   DIAGNOSTIC bits, results are WRONG.  fp32 / bf16 kernels: 1 skip LayerNorm/act, 2 skip weight
 *                  DMA, 4 skip barriers (tools/tune_mlp.py); feature-split bf16 kernel: 1 weights from chunk 0 only,
 *                  2 skip LayerNorm/act, 4 load only the first input panel, 8 skip the per-panel barriers, 16 LDS
 *                  operand reads from chunk 0 only (tools/tune_mlp_split.py)
 *   "mlp_split3_rows128" tile shape of hgnn_mlp_forward_f32_split3 for K -> 512 -> 256 at M >= 65,536: 1 (default)
 *                  128-row tiles, 8 waves, hidden rows consumed in two K-halves; 0 the 64-row kernel that serves every
 *                  other shape; 2 EXPERIMENTAL 64-row tiles, 4 waves, two workgroups per CU -- fastest, but one of two
 *                  equivalent builds returned wrong elements, cause not found: never a default, and
 *                  refused unless the environment variable HGNN_EXPERIMENTAL is set
 *   "mlp_split3_one_wg"  DIAGNOSTIC: 1 launches one persistent workgroup per CU where two fit (results must be
 *                  bitwise the same: tests/test_gpu_split3.py)
 *   "k1_one_launch" 1 (default): in hgnn_segment_reduce_f32_ex the chunk of a split destination that arrives last
 *                  sums its partial rows, and no combine launch follows; 0 the two launches of hgnn_segment_reduce_f32
 *   "k1_item_order" 0 (default): plan order; 1: hgnn_segment_reduce_f32_ex hands the work items out in the order
 *                  it is given (hgnn_plan_item_order: longest lists first).  Off until a measurement shows that it
 *                  pays.  Results do not depend on either option.
 * Any other name is an error (HGNN_ERR_INVALID_ARG). */
int hgnn_set_option(const char* name, int value);
/* the current value of an option */
int hgnn_get_option(const char* name, int* value);

/* Fills n_rows/n_dst/n_src/chunk/max_* of `plan` (pointers untouched).
 * chunk <= 0 selects the default rule (quarter of a wave's share of the rows,
 * clamped to [32, 512]). */
int hgnn_plan_dims(int64_t n_rows, int64_t n_dst, int64_t n_src, int32_t chunk, hgnn_plan* plan);

/* Bytes of scratch hgnn_plan_build needs (device memory, any 256-B aligned). */
int hgnn_plan_workspace_bytes(int64_t n_rows, int64_t n_dst, size_t* bytes);

/* dst_index: int64[M] destinations (PyG edge_index row / bipartite_graph row).
 * gather_index: int64[M] source-table rows, or NULL (row e of the table is edge e).
 * Out-of-range entries are dropped and flagged in counts[HGNN_CNT_ERR]. */
int hgnn_plan_build(const int64_t* dst_index, const int64_t* gather_index, hgnn_plan* plan,
                    void* workspace, size_t workspace_bytes, hgnn_stream_t stream);

/* out[d,:] = sum_{p in list(d)} weight[perm[p]] * row_scale[src_row[p]] * src[src_row[p],:]
 * weight (float[M], by ORIGINAL position) and row_scale (float[n_src]) may be NULL.
 * out: float[N,F] (every row written, zeros for empty lists);
 * partial: float[max_partial,F] scratch.  Deterministic: fixed summation order. */
int hgnn_segment_reduce_f32(const hgnn_plan* plan, const float* src, int32_t F,
                            const float* weight, const float* row_scale,
                            float* out, float* partial, hgnn_stream_t stream);

/* The same sums, bit for bit, with two device arrays that are not part of hgnn_plan:
 *   arrive  int32[max(plan->max_split, 1)], all zero when first handed in and left all zero by every call.  Plain
 *           fp32 rows of 4-element columns (no weight, F % 4 == 0, F <= 1024) then need ONE launch: each chunk of
 *           a split destination adds to arrive[split] once its partial row is out, and the chunk that arrives last
 *           sums the partial rows, in chunk order, into the output row.  No wave waits for another.  Every other
 *           form runs the two launches of hgnn_segment_reduce_f32.
 *   order   int32[plan->max_work] from hgnn_plan_item_order, or NULL for plan order (same forms as above).
 * `partial` and `arrive` belong to one call at a time: two calls on one plan that may overlap (different streams)
 * need buffers of their own, as they always did for `partial`. */
int hgnn_segment_reduce_f32_ex(const hgnn_plan* plan, const float* src, int32_t F,
                               const float* weight, const float* row_scale, float* out, float* partial,
                               int32_t* arrive, const int32_t* order, hgnn_stream_t stream);

/* order[0 .. max_work): the work items of a built plan by non-increasing list length in buckets of 8 rows,
 * plan order kept inside a bucket; entries past counts[HGNN_CNT_WORK] hold indices >= that count.  Long lists
 * that start late keep a launch open while most of the chip is idle; this starts them first.  Built once per plan.
 * workspace: device scratch of hgnn_plan_item_order_workspace_bytes (needs the plan's dims only). */
int hgnn_plan_item_order_workspace_bytes(const hgnn_plan* plan, size_t* bytes);
int hgnn_plan_item_order(const hgnn_plan* plan, int32_t* order, void* workspace, size_t workspace_bytes,
                         hgnn_stream_t stream);

/* Segmented min / max with arg output, and exact integer sums, over a plain destination plan (no gather index):
 * torch_scatter.scatter_min / scatter_max (BipartiteClassification/bipartite_classification_base.py:158,
 * gMRT/gmrt_base.py:165, tracking_utils.py:41) and the integer scatter_sum of tracking_utils.py:37.
 *   op     HGNN_RED_MIN / HGNN_RED_MAX: out[d,f] = the min / max of src[e,f] over the rows e of list d,
 *          arg[d,f] (int64) = that row e.  Ties go to the smallest e (first occurrence); NaN is never
 *          selected (a list holding only NaN is empty); +-inf are ordinary values.  Empty lists: out = 0,
 *          arg = n_rows.  Values are compared exactly in their own type (bf16 without rounding, int64 as
 *          64-bit integers); the result does not depend on the plan's chunk.
 *          HGNN_RED_SUM (dtype I32 / I64 only; arg unused, may be NULL): out[d,f] = the wrapping integer sum.
 *          Floating-point sums are hgnn_segment_reduce_f32 / _bf16 (HGNN_ERR_UNSUPPORTED here).
 *   dtype  HGNN_DT_F32 / _BF16 / _I32 / _I64: the element type of src, out and partial.
 *   src    [n_rows, F], out [n_dst, F] (every element written), arg int64 [n_dst, F];
 *   partial      scratch of plan->max_partial * F elements of dtype,
 *   partial_arg  int32 scratch of plan->max_partial * F elements (MIN / MAX only; NULL for SUM).
 * Rows of 4-element columns (F % 4 == 0, F <= 1024, 16-byte aligned pointers; 8-byte for bf16) take the
 * vector path, any other shape a row-parallel path.  Deterministic: no atomics, each element written once. */
#define HGNN_RED_SUM 0
#define HGNN_RED_MIN 1
#define HGNN_RED_MAX 2
#define HGNN_DT_F32 0
#define HGNN_DT_BF16 1
#define HGNN_DT_I32 2
#define HGNN_DT_I64 3
#define HGNN_DT_F64 4   /* hgnn_graph_intersection weights only (ABI 26) */
int hgnn_segment_reduce_ex(const hgnn_plan* plan, int32_t op, int32_t dtype, const void* src, int32_t F,
                           void* out, int64_t* arg, void* partial, int32_t* partial_arg, hgnn_stream_t stream);

/* Backward of the min / max above: grad_src[arg[d,f], f] = grad_out[d,f] where 0 <= arg[d,f] < n_rows, and 0
 * everywhere else (grad_src [n_rows, F] is cleared first).  Each element receives at most one value: no atomics.
 * dtype HGNN_DT_F32 or HGNN_DT_BF16 (integer src is not differentiable). */
int hgnn_segment_arg_backward(const int64_t* arg, int64_t n_dst, int32_t F, int64_t n_rows, int32_t dtype,
                              const void* grad_out, void* grad_src, hgnn_stream_t stream);

/* out[e,:] = weight[e] * row_scale[idx[e]] * table[idx[e],:]   (idx[e] < 0 -> zeros)
 * idx: int32[M]; weight float[M] / row_scale float[table_rows] may be NULL. */
int hgnn_gather_rows_f32(const float* table, int64_t table_rows, int32_t F,
                         const int32_t* idx, int64_t M,
                         const float* weight, const float* row_scale,
                         float* out, hgnn_stream_t stream);

/* The transpose of hgnn_segment_reduce_f32 (= backward of scatter_add, and the row gather
 * table[index] when the plan was built on `index`):
 *     out[e,:] = weight[e] * table[dst(e),:]      for every row e of the plan
 * walked in DESTINATION order: each table row is read once and written to the rows of its
 * list, so HBM sees one pass of 16-B stores over out[M,F] instead of M random row reads.
 * weight (float[M], by original position) may be NULL.  Rows whose index was out of range
 * are not written. */
int hgnn_spread_rows_f32(const hgnn_plan* plan, const float* table, int32_t F,
                         const float* weight, float* out, hgnn_stream_t stream);

/* bf16 feature rows (BASELINE config 4 dtype): same semantics as the _f32 entry points with
 * bf16 src/table/out (16-byte aligned, F a multiple of 8, F <= 512), fp32 accumulation and one
 * rounding per output element; weight / row_scale stay fp32; `partial` is fp32[max_partial,F]. */
int hgnn_segment_reduce_bf16(const hgnn_plan* plan, const void* src, int32_t F, const float* weight,
                             const float* row_scale, void* out, float* partial, hgnn_stream_t stream);
int hgnn_spread_rows_bf16(const hgnn_plan* plan, const void* table, int32_t F, const float* weight,
                          void* out, hgnn_stream_t stream);
int hgnn_gather_rows_bf16(const void* table, int64_t table_rows, int32_t F, const int32_t* idx, int64_t M,
                          const float* weight, void* out, hgnn_stream_t stream);

/* out[e] = sum_f A[ai[e],f] * B[bi[e],f];  ai/bi int32[M] or NULL (identity);
 * negative index -> 0. */
int hgnn_edge_dot_f32(const float* A, const int32_t* ai, int64_t a_rows,
                      const float* B, const int32_t* bi, int64_t b_rows,
                      int32_t F, int64_t M, float* out, hgnn_stream_t stream);

/* int64 -> int32 index conversion with range check (out-of-range -> -1, err flag set) */
int hgnn_index_to_i32(const int64_t* idx, int64_t M, int64_t limit, int32_t* out,
                      int32_t* err_flag, hgnn_stream_t stream);

/* Fixed-radius kNN (exact, tiled brute force) in a D<=16 dimensional space: for every query
 * the <=K nearest points with squared distance < radius^2, ascending (ties: lower index first),
 * idx -1 padded; dist2_out (may be NULL) holds squared distances, -1 for padding.
 * Replaces frnn.frnn_grid_points as called by find_neighbors (Modules/utils.py:228-239) from
 * DynamicGraphConstruction.forward (Modules/gnn_utils.py:194).  K in {1-6,8,10,12,16,20,32} or any K in
 * [33, 128] (ABI 26; the embedding stage's FRNN_graph, knn: 100).  Exactly: the K smallest (d2, idx) pairs in
 * lexicographic order among the points with d2 < radius^2 (radius^2 rounded in float32), so a K = 64 call's first
 * 32 columns equal a K = 32 call bit for bit.  This entry accepts K > 32 too (one pass, no candidate split). */
int hgnn_knn_radius_f32(const float* query, int64_t nq, const float* points, int64_t np, int32_t D,
                        int32_t K, float radius, int64_t* idx_out, float* dist2_out, hgnn_stream_t stream);

/* Same search with (i) the radius optionally read from DEVICE memory (`radius_dev` != NULL: the module's
 * knn_radius buffer, Modules/gnn_utils.py:181,205 -- no host read of it) and (ii) a workspace that lets a
 * search with few queries (the S x S super graph) split every query's candidates across workgroups and
 * merge the per-slice lists afterwards (same result, ties included).  workspace may be NULL (no split). */
int hgnn_knn_workspace_bytes(int64_t nq, int64_t np, int32_t K, size_t* bytes);
int hgnn_knn_radius_ws_f32(const float* query, int64_t nq, const float* points, int64_t np, int32_t D,
                           int32_t K, float radius, const float* radius_dev, int64_t* idx_out, float* dist2_out,
                           void* workspace, size_t workspace_bytes, hgnn_stream_t stream);

/* The same search -- the K smallest (d2, idx) pairs with d2 < radius^2, bit for bit what the two entries above
 * return -- without comparing every query with every point (csrc/knn_sorted.hip): the points are sorted along a
 * Morton curve and cut into tiles of 256 with a box each, 16 curve-consecutive queries visit the tiles from their
 * home tile outwards and skip a tile whose box is provably too far ("k_knn_sorted").  EVERY K in
 * [1, 128], D in [1, 16], nq != np allowed; query == points with nq == np shares one sort.  All stages run on
 * `stream` from `workspace` (hgnn_knn_sorted_workspace_bytes; 16-byte aligned; required): no host read, no
 * allocation.  After the call the int64[2] at workspace offset 0 holds {tiles visited, tiles skipped} summed over
 * the workgroups (visited + skipped = workgroups x tiles); `stats_out` (device int64[2], may be NULL) receives a
 * copy.  nq == 0 returns HGNN_OK; np == 0 fills the outputs with -1. */
int hgnn_knn_sorted_workspace_bytes(int64_t nq, int64_t np, int32_t D, int32_t K, size_t* bytes);
int hgnn_knn_radius_sorted_f32(const float* query, int64_t nq, const float* points, int64_t np, int32_t D,
                               int32_t K, float radius, const float* radius_dev, int64_t* idx_out,
                               float* dist2_out, void* workspace, size_t workspace_bytes,
                               int64_t* stats_out, hgnn_stream_t stream);

/* ------------------------------------------------------------------------
 * The hierarchy decision of HierarchicalGNNBlock.clustering
 * (BipartiteClassification/Models/HGNN_GMM.py:162-234) without host round trips.
 *
 * hgnn_gmm2_fit_f32: 2-component 1-D Gaussian mixture of v[M] (the atanh edge likelihoods, :188-189), what
 *   the reference gets from sklearn GaussianMixture(2).fit on the CPU (:192).  Deterministic 2-means start
 *   from the data extremes, then at most max_iter EM passes with sklearn's stopping rule (change of the mean
 *   log-likelihood < tol; reg_covar added to the variances) evaluated ON THE DEVICE: all passes are enqueued,
 *   the ones after convergence return immediately.  As in sklearn, n_k += 10 eps(float32) and the weights are
 *   n_k / (n_0 + n_1): they sum to 1 for any M.  M >= 1, 1 <= max_iter <= 1000, tol >= 0 and reg_covar > 0
 *   (a component of identical values has variance exactly reg_covar, and the E step divides by it; 0 is
 *   refused with HGNN_ERR_INVALID_ARG).  state: double[HGNN_GMM_STATE] =
 *   {w0, w1, mu0, mu1, var0, var1, previous lower bound, converged, EM passes run, min, max, c0, c1, cut,
 *    last lower bound, -};  partials: double[HGNN_GMM_BLOCKS * 8] scratch;  ticket: one uint32 scratch.
 * hgnn_gmm2_cut_f32: the cut x between the two means where sigmoid(r) P(left|x) = sigmoid(-r) P(right|x)
 *   (:162-170, scipy fsolve in the reference; bisection here) -> state[13]; then, on the module's DEVICE
 *   buffer score_cut[1] (:157): inf -> middle of the means (:196-197); in training mode, if the cut lies
 *   between the means, score_cut = momentum * score_cut + (1 - momentum) * cut (:201-208).
 * hgnn_cc_labels: weakly connected components over vertices 0..n-1 of the edges (src[e], dst[e]) whose
 *   score[e] >= *cut (score == cut == NULL: all edges), :212-221 (cugraph in the reference).  labels[v] =
 *   smallest vertex id of v's component (v itself if isolated); present[v] = 1 iff v is an endpoint of a
 *   kept edge.  Edges with a NaN score or an endpoint outside [0, n) are dropped.  score and cut are given
 *   together or not at all; with M = 0 (src, dst and score may be NULL) a cut alone is accepted and every
 *   vertex is its own component.  Lock-free union-find: one pass over the edges, one compression pass; no
 *   iteration to convergence and therefore no host read.
 * ------------------------------------------------------------------------ */
#define HGNN_GMM_STATE 16
#define HGNN_GMM_BLOCKS 1024
int hgnn_gmm2_fit_f32(const float* v, int64_t M, int32_t max_iter, float tol, float reg_covar, double* state,
                      double* partials, uint32_t* ticket, hgnn_stream_t stream);
int hgnn_gmm2_cut_f32(double* state, float granularity, int32_t training, float momentum, float* score_cut,
                      hgnn_stream_t stream);
int hgnn_cc_labels(const int64_t* src, const int64_t* dst, int64_t M, int64_t n, const float* score,
                   const float* cut, int32_t* labels, int32_t* present, hgnn_stream_t stream);

/* ------------------------------------------------------------------------
 * Fused gather -> concat -> Linear -> LayerNorm -> act -> ... -> (+skip) MLP
 * (fp32 MFMA).  One descriptor describes up to 3 concatenated input segments,
 * each an optional row gather of a table, and up to 3 Linear layers with
 * LayerNorm + activation after each (make_mlp with layer_norm=True,
 * reference Modules/utils.py:169-196), as instantiated for the edge / node /
 * supernode / superedge networks at Modules/gnn_utils.py:22-41 and :77-115,
 * fused with the concat + gathers feeding them (:52,:61,:126,:134,:144,:152)
 * and the skip connection (:53,:62,:126,:134,:144,:152).  "K6+K7".
 * ------------------------------------------------------------------------ */
#define HGNN_ACT_NONE 0
#define HGNN_ACT_GELU 1 /* erf form, nn.GELU() default */
#define HGNN_ACT_TANH 2
#define HGNN_ACT_RELU 3
/* 4..7: the torch.nn classes make_mlp is given by name, at their constructor defaults (the reference builds them with
 * no arguments).  Forms and error bounds: csrc/mlp_common.h */
#define HGNN_ACT_SILU 4       /* x * sigmoid(x), nn.SiLU()                                 */
#define HGNN_ACT_LEAKY_RELU 5 /* negative_slope = 0.01, nn.LeakyReLU()                     */
#define HGNN_ACT_ELU 6        /* alpha = 1.0, nn.ELU()                                     */
#define HGNN_ACT_SIGMOID 7    /* nn.Sigmoid()                                              */
#define HGNN_ACT_LAST HGNN_ACT_SIGMOID /* the entries refuse a code above this one         */

typedef struct hgnn_mlp_desc {
    int32_t n_seg;               /* 1..3 input segments, concatenated in order    */
    const float* seg_table[3];   /* [rows_i, seg_width[i]]                        */
    const int32_t* seg_index[3]; /* int32[M] row gather, or NULL (row e)          */
    int32_t seg_width[3];
    int32_t n_layers;            /* 1..3 (1: see hgnn_mlp_supported, single layers) */
    const float* W[3];           /* Linear weight [out_i, in_i] row-major (torch) */
    const float* b[3];           /* [out_i]                                       */
    const float* ln_w[3];        /* LayerNorm affine, NULL = no LayerNorm         */
    const float* ln_b[3];
    int32_t width[4];            /* in, h1, (h2), out                             */
    int32_t act[3];              /* HGNN_ACT_* after each layer                   */
    float ln_eps;
    const float* skip;           /* [M, out] added to the result, or NULL         */
    int64_t M;                   /* rows                                          */
    int32_t w0_cols;             /* columns stored per row of W[0]: 0 = width[0]; must be 16 (zero
                                  * padded) in small-K mode, i.e. when width[0] <= 16 is not a
                                  * multiple of 16 (node / edge encoders, K = 3 / 6: IN.py:26-46)  */
    int32_t w_last_rows;         /* rows stored in the last W / b (and ln_w / ln_b): 0 = width[n].  Must be 32
                                  * (zero padded) for a head = plain last layer of width[n] <= 32 real outputs
                                  * (width-1 classifiers IN.py:107-115, HGNN_GMM.py:313-321; emb_dim-wide
                                  * embedding head HGNN_GMM.py:74-82), and P = width[1] / 2 (zero padded) for a
                                  * LayerNorm'ed last layer of P-16 < width[n] < P outputs (supernode encoder,
                                  * L - emb_dim wide, HGNN_GMM.py:117): statistics and stores use width[n] */
    float* save_pre[3];          /* optional: [M, width[l+1]] buffers that receive layer l's output
                                  * BEFORE LayerNorm/activation (what a backward pass needs; hidden
                                  * activations are recomputed from it).  NULL = not saved.         */
    int32_t n_pre;               /* 0..2 PRE-PROJECTED gathered segments (fp32 kernel and bf16 split kernel): a gathered
                                  * segment table[idx] enters the first Linear linearly,
                                  *   W_s table[idx[e]] = (table W_s^T)[idx[e]],
                                  * so the caller may project the (few) table rows once, P_s = table W_s^T
                                  * [rows, width[1]], leave the segment out of seg_* / W[0] / width[0], and
                                  * hand P_s here: the kernel starts row e's accumulators at
                                  * b + sum_s P_s[pre_index[s][e]].  For nodes[graph[k]] (N rows, M = 16.7 N
                                  * edges) this removes 2/3 of the edge network's first-layer FLOPs.  */
    const float* pre_table[2];   /* [rows_s, width[1]], 16-byte aligned (bf16 rows for
                                  * hgnn_mlp_forward_bf16_split)                    */
    const int32_t* pre_index[2]; /* int32[M]                                      */
} hgnn_mlp_desc;

/* 1 if hgnn_mlp_forward_f32 has an instantiation for this descriptor (host-only check):
 *   cell networks / encoders: widths K -> 2L (-> 2L) -> L, LayerNorm on every layer,
 *       L in {32, 64, 128, 256}; every segment a multiple of 16 floats wide, or K <= 16 in
 *       small-K mode (W[0] zero-padded to 16 columns, w0_cols = 16);
 *   heads: K -> H -> H -> w, 1 <= w <= 32, LayerNorm + activation on the two hidden layers, plain last
 *       layer (ln_w[2] = NULL, act[2] = NONE) stored zero-padded as 32 rows (w_last_rows = 32),
 *       H in {64, 128, 256, 512}, no skip; out is float[M, w];
 *   single layers: n_layers = 1, K -> o with o in {512, 1024}, LayerNorm + activation (+ skip): the pieces of an
 *       fp32 MLP at latent 512 (its 1024-wide hidden layer is 256 accumulators per lane: one launch per layer, the
 *       hidden rows make one trip through HBM); save_pre[0] dumps the pre-LayerNorm rows (training forward of the
 *       encoders' first Linear).  Narrow single layer (inference): 496 < o < 512, o % 4 == 0, W / b / ln_w / ln_b
 *       zero padded to 512 rows (w_last_rows = 512), no skip, no save_pre: LayerNorm over the o real features,
 *       out is float[M, o] (the last layer of the supernode encoder at latent 512);
 *   narrow encoders: K -> 2P -> 2P -> o with P in {32, 64, 128, 256}, P-16 < o < P, o % 4 == 0, the last
 *       layer's W / b / ln_w / ln_b zero padded to P rows (w_last_rows = P), no skip, no save_pre;
 *       LayerNorm over the o real features; out is float[M, o]. */
int hgnn_mlp_supported(const hgnn_mlp_desc* d);

/* out[M, L] = MLP(cat_i seg_i[idx_i]) (+ skip).  No workspace; hidden activations stay in
 * registers.  Negative gather indices read row 0 (callers validate indices at plan build). */
int hgnn_mlp_forward_f32(const hgnn_mlp_desc* d, float* out, hgnn_stream_t stream);

/* Widths BETWEEN the grid's (a latent / hidden_ratio sweep: latent 48, 96, 160, 192, hidden = 3 x latent, ...): the
 * same exact-fp32 kernel on the instantiation of the next grid width, with zero-padded parameters.
 *   cell networks / encoders: K -> h (-> h) -> o, LayerNorm on every layer, h % 16 == 0, 32 <= h <= 512,
 *       o % 4 == 0, 4 <= o <= h / 2; segments as for hgnn_mlp_supported (multiples of 16, or small-K mode); skip,
 *       n_pre and save_pre allowed;
 *   heads: K -> H -> H -> w, plain last layer of 1 <= w <= 32 outputs, H % 16 == 0, 32 <= H <= 512, no skip,
 *       save_pre[0..1] allowed.
 * Let P = the smallest of {32, 64, 128, 256} with 2P >= h (heads: >= H).  width[] carries the REAL widths; the storage
 * the kernel reads follows from them:
 *   W[0]            [2P, K]  rows h .. 2P-1 zero (K = width[0], or w0_cols = 16 columns in small-K mode);
 *   W[1] (3 layers) [2P, 2P] rows and columns h .. 2P-1 zero;
 *   last W          [P, 2P]  rows o .. P-1 and columns h .. 2P-1 zero (heads: [32, 2P], rows w .. 31 zero);
 *   b, ln_w, ln_b of every layer: as many entries as the layer's W has rows, the padded ones ZERO (ln_w too: a padded
 *       feature must come out as 0, it is the next layer's input);
 *   w_last_rows = P (heads: 32), checked;
 *   pre_table[s]    [rows, 2P] = table W_s^T with the padded W[0]: columns h .. 2P-1 zero.
 * LayerNorm statistics run over the real features only (padded ones are masked out of the centred pass).  Rows in
 * HBM have their real widths: skip and out are [M, o], save_pre[l] is [M, width[l+1]].
 * The check accepts grid shapes too (no padding); hgnn_mlp_supported / hgnn_mlp_forward_f32 do not read this layout. */
int hgnn_mlp_supported_f32_padded(const hgnn_mlp_desc* d);
int hgnn_mlp_forward_f32_padded(const hgnn_mlp_desc* d, float* out, hgnn_stream_t stream);

/* Networks WITHOUT LayerNorm (make_mlp with layer_norm=False, the reference's default): the same exact-fp32 kernel
 * with the statistics left out, each layer act[l](x W^T + b).  Same descriptor; ln_w[l] == ln_b[l] == NULL on EVERY
 * layer (a network that mixes LayerNorm'ed and plain layers is refused here; hgnn_mlp_supported keeps refusing a plain
 * hidden layer).  ln_eps is not read.  act[l] in HGNN_ACT_NONE .. HGNN_ACT_LAST.  Shapes: the multi-layer grid shapes of
 * hgnn_mlp_supported --
 *   cell networks / encoders: K -> 2L (-> 2L) -> L, L in {32, 64, 128, 256}; segments multiples of 16, or K <= 16 in
 *       small-K mode (w0_cols = 16); skip, n_pre and save_pre allowed; w_last_rows = 0 (or L);
 *   heads: K -> H -> H -> w, 1 <= w <= 32, act[2] = HGNN_ACT_NONE, the last W / b stored zero padded as 32 rows
 *       (w_last_rows = 32), H in {64, 128, 256, 512}, no skip, save_pre[0..1] allowed; out is float[M, w];
 *   narrow encoders: K -> 2P -> 2P -> o, P in {32, 64, 128, 256}, P - 16 < o < P, o % 4 == 0, the last W / b zero
 *       padded to P rows (w_last_rows = P: here only a store mask), no skip, no save_pre; out is float[M, o].
 * save_pre[l] receives layer l's pre-activation rows z_l = x W^T + b.  Single layers, the padded widths and the
 * split-bf16 / bf16 kernels have no plain form. */
int hgnn_mlp_supported_f32_plain(const hgnn_mlp_desc* d);
int hgnn_mlp_forward_f32_plain(const hgnn_mlp_desc* d, float* out, hgnn_stream_t stream);

/* SQUARE networks: the output as wide as the hidden layers (hidden_ratio 1, hidden == latent), and single layers below
 * 512 -- the same exact-fp32 kernel, instantiated with equal tile counts (csrc/mlp_fused_square.hip).  Same descriptor
 * and segment rules as hgnn_mlp_supported (multiples of 16, or small-K mode with w0_cols = 16; n_pre allowed); fp32
 * rows, LayerNorm on EVERY layer.  Let h = width[1] (n_layers = 1: the output width), h % 16 == 0, 32 <= h <= 256, and
 * P = the smallest of {32, 64, 128, 256} with P >= h.
 *   square:  K -> h (-> h) -> h, n_layers 2 or 3; skip and save_pre allowed;
 *   narrow:  K -> h -> h -> o with h - 16 < o < h, o % 4 == 0 (the supernode encoder at hidden == latent); no skip, no
 *            save_pre; out is float[M, o];
 *   single:  K -> h, one Linear -> LayerNorm -> act (+ skip); save_pre[0] allowed.
 * width[] carries the REAL widths.  Storage:
 *   h == P and o == h (square / single on the grid): the parameters as they are; w_last_rows = 0 (or h);
 *   otherwise (PAD kernels): every layer's W, b, ln_w, ln_b zero padded to P rows (ln_w too), W[l >= 1] also to P
 *       columns ([P, P]; W[0] is [P, K] or [P, 16]), pre_table[s] is [rows, P] with columns h .. P-1 zero,
 *       w_last_rows = P, checked.  LayerNorm statistics are masked to the real features; skip, out and save_pre[l]
 *       rows have their real widths.
 * Not here: h > 256 (512 / 1024 are hgnn_mlp_supported's single layers), h / 2 < o <= h - 16, heads, bf16 rows.  No
 * shape of this entry is accepted by another hgnn_mlp_supported*; their verdicts do not depend on it. */
int hgnn_mlp_supported_f32_square(const hgnn_mlp_desc* d);
int hgnn_mlp_forward_f32_square(const hgnn_mlp_desc* d, float* out, hgnn_stream_t stream);

/* bf16 variant (BASELINE config 4 dtype) on v_mfma_f32_16x16x32_bf16.  Same descriptor, read as:
 * seg_table / skip / out = bf16 rows; W[l] = bf16 [out][in] row-major, and for l >= 1 with its
 * COLUMNS stored in MFMA k-slot order: column 32c + 8g + j holds input feature
 * 32c + (j < 4 ? 4g + j : 16 + 4g + j - 4)  (c = k-block, g = 0..3, j = 0..7);
 * b / ln_w / ln_b fp32; accumulation and LayerNorm in fp32.  Supported: K -> 2L (-> 2L) -> L,
 * LayerNorm on every layer, L in {32, 64, 128, 256}, every segment a multiple of 32 wide. */
int hgnn_mlp_supported_bf16(const hgnn_mlp_desc* d);
int hgnn_mlp_forward_bf16(const hgnn_mlp_desc* d, void* out, hgnn_stream_t stream);

/* bf16, feature-split kernel for the wide layers (L in {128, 256, 512}; config 4 is L = 512): a
 * workgroup owns 64 rows, each of its 4 waves a quarter of every layer's features; hidden
 * activations cross waves through LDS, weights go straight from L2 to registers.  Same descriptor
 * and arithmetic as hgnn_mlp_forward_bf16, except that W[l] (bf16) is stored in MFMA A-FRAGMENT
 * ORDER, natural feature order for every layer:
 *   element index = ((c * (F/16) + T) * 64 + lane) * 8 + i  holds  W[16T + lane%16][32c + 8(lane/16) + i]
 * (F = out features, c = 32-wide k-chunk, T = 16-feature tile, lane = 0..63, i = 0..7).
 * Supported: K -> 2L (-> 2L) -> L, LayerNorm on every layer, every segment a multiple of 128 wide; and single layers
 * (n_layers = 1) K -> o, o in {256, 512, 1024}, LayerNorm + activation (+ skip): the pieces from which the heads and
 * the encoder tails (bf16 latent mode) are chained.
 * save_pre[l] (optional) receives layer l's pre-LayerNorm rows as BF16 [M, width[l+1]] (8-byte aligned): the
 * forward of the bf16 training path. */
int hgnn_mlp_supported_bf16_split(const hgnn_mlp_desc* d);
int hgnn_mlp_forward_bf16_split(const hgnn_mlp_desc* d, void* out, hgnn_stream_t stream);

/* fp32 rows, SPLIT-bf16 arithmetic (the Python layer's default path of the fp32 MLPs at latent 128 / 256: K -> 2L (-> 2L) -> L, and
 * K -> H -> H with H in {256, 512} = the two hidden layers of a score head, whose plain last Linear the caller applies;
 * LayerNorm on every layer, every segment a multiple of 128 wide, n_pre allowed, save_pre optional (fp32 dumps)): every fp32 operand of
 * the GEMMs is used as hi + mid with hi = bf16(x), mid = bf16(x - hi), and  x.w ~= hi.hi + mid.hi + hi.mid  runs as
 * three v_mfma_f32_16x16x32_bf16 (exact products, fp32 accumulation) instead of one fp32 MFMA at 1/16 of the rate.
 * Bias, LayerNorm, exact-erf GELU / tanh, skip and every row in HBM stay fp32.  Error at model level 2e-5 against the
 * reference's scores on BASELINE config 2 (north_star's bar: 1e-4).  Same descriptor as hgnn_mlp_forward_f32 (fp32
 * segment tables, fp32 pre_table rows of width[1] floats, fp32 skip / out), except W[l]: bf16, the layer's split
 * stream -- per 32-wide k-chunk c of the (kept) input columns the chunk's W_hi columns followed by its W_mid columns,
 * i.e. a [out, 2 K] matrix whose 32-column chunks 2c / 2c + 1 are hi / mid -- in the A-fragment order of
 * hgnn_mlp_forward_bf16_split. */
int hgnn_mlp_supported_f32_split3(const hgnn_mlp_desc* d);
int hgnn_mlp_forward_f32_split3(const hgnn_mlp_desc* d, float* out, hgnn_stream_t stream);

/* The SPLIT-bf16 arithmetic of hgnn_mlp_forward_f32_split3 at widths BETWEEN its two (latent 96, 144, 160, 192,
 * hidden = 3 x latent, ...): its 64-row kernel on zero-padded, split parameters.  No-grad forward, opt-in in the Python
 * layer (fused.set_split3_padded).
 *   cell networks only: K -> h (-> h) -> o, 2 or 3 layers, LayerNorm on every layer, fp32 rows, h % 16 == 0,
 *       128 < h <= 512, o % 4 == 0, 4 <= o <= h / 2; 1..3 segments, each a positive multiple of 16 wide (no small-K
 *       mode); skip and n_pre <= 2 allowed; save_pre refused; M < 2^31.
 * Let P = 128 when h <= 256, else 256 (the 4-wave / 8-wave instantiations: 2P hidden and P output features stored).
 * width[] and seg_width[] carry the REAL widths; the storage the kernel reads follows from them, as for
 * hgnn_mlp_forward_f32_padded:
 *   W[0]            [2P, Kp] rows h .. 2P-1 zero; Kp: each kept segment's column block zero padded to the next multiple
 *                   of 128 columns (a segment w wide is ceil(w / 128) input panels);
 *   W[1] (3 layers) [2P, 2P] rows and columns h .. 2P-1 zero;
 *   last W          [P, 2P]  rows o .. P-1 and columns h .. 2P-1 zero;
 *   each padded W is then stored as its split stream (hi / mid chunks in A-fragment order), exactly as
 *       hgnn_mlp_forward_f32_split3 reads an unpadded one;
 *   b, ln_w, ln_b of every layer: as many fp32 entries as the layer's W has rows, the padded ones ZERO (ln_w too: a
 *       padded feature must come out as 0, it is the next layer's input);
 *   w_last_rows = P, checked (w0_cols = 0);
 *   pre_table[s]    fp32 [rows, 2P] = table W_s^T, columns h .. 2P-1 zero.
 * Rows in HBM keep their real widths and strides: segment tables [rows, seg_width[s]] (a 16-byte piece past a
 * segment's width is never read), skip and out [M, o].  LayerNorm statistics run over the real features only: every
 * wave centres its own real features, the waves' (mean, M2) pairs are pooled with their real counts, which may be 0.
 * The check accepts the grid shapes K -> 2L (-> 2L) -> L, L in {128, 256}, too (segments then multiples of 16 rather
 * than 128); on a descriptor both entries accept -- up to w_last_rows -- this one returns the bits of
 * hgnn_mlp_forward_f32_split3's 64-row kernel. */
int hgnn_mlp_supported_f32_split3_padded(const hgnn_mlp_desc* d);
int hgnn_mlp_forward_f32_split3_padded(const hgnn_mlp_desc* d, float* out, hgnn_stream_t stream);

/* out[M, N] = x[M, K] . W^T (+ skip), all fp32 in HBM, the product as split-bf16 (same arithmetic and the same
 * weight stream layout as hgnn_mlp_forward_f32_split3: w_split = the split stream of W [N, K]): the M-row data-gradient
 * GEMMs of the fp32 training backward.  K a multiple of 128, N in {256, 512}; skip [M, N] or NULL. */
int hgnn_linear_f32_split3(const float* x, int64_t M, int32_t K, const void* w_split, int32_t N,
                           const float* skip, float* out, hgnn_stream_t stream);

/* The pre-projections of an edge update in ONE launch: out_s[M, N] = x[M, K] . W_s^T for s = 0 (and 1, when w_split1 /
 * out1 are given) over the same input rows (x = the node table, W_s = the first Linear's column block of gathered
 * segment s; hgnn_mlp_desc.pre_table).  Same split-bf16 arithmetic as hgnn_mlp_forward_f32_split3 itself (three
 * products), same weight stream layout as hgnn_linear_f32_split3.  K a multiple of 128, N in {256, 512}. */
int hgnn_project_f32_split3(const float* x, int64_t M, int32_t K, const void* w_split0, const void* w_split1,
                            int32_t N, float* out0, float* out1, hgnn_stream_t stream);

/* LayerNorm + activation of one make_mlp layer (Modules/utils.py:169-196: Linear -> LayerNorm ->
 * act) over rows z[M, W] (the Linear's output, as dumped by hgnn_mlp_forward_f32's save_pre), one
 * pass each -- the elementwise half of the fused MLP's backward (the GEMM half is the library's, or both halves in one
 * launch: hgnn_mlp_backward_layer_f32 below):
 *   forward :  out[r]    = act(gamma * (z[r] - mean_r) * rstd_r + beta)
 *   backward:  grad_z[r] = d/dz of the above applied to grad_out[r]; and per-workgroup column sums
 *              partials[b][0][c] = sum_r grad_y * xhat (dgamma), [b][1][c] = sum_r grad_y (dbeta),
 *              [b][2][c] = sum_r grad_z (gradient of the Linear's bias); the caller adds the
 *              HGNN_LN_ACT_BLOCKS partial rows (deterministic, no atomics).
 * W in {64, 128, 256, 512, 1024}; act = HGNN_ACT_*; exact-erf GELU as in the forward kernels. */
#define HGNN_LN_ACT_BLOCKS 1024
int hgnn_ln_act_forward_f32(const float* z, int64_t M, int32_t W, const float* gamma, const float* beta,
                            int32_t act, float eps, float* out, hgnn_stream_t stream);
int hgnn_ln_act_backward_f32(const float* z, const float* grad_out, int64_t M, int32_t W, const float* gamma,
                             const float* beta, int32_t act, float eps, float* grad_z,
                             float* partials /* [HGNN_LN_ACT_BLOCKS][3][W] */, hgnn_stream_t stream);

/* The LayerNorm-less twins (a layer of hgnn_mlp_forward_f32_plain; z as dumped by its save_pre), same kernel body,
 * same widths and alignment rules:
 *   forward :  out[r]    = act(z[r])
 *   backward:  grad_z[r] = grad_out[r] * act'(z[r]); partials[b][c] = workgroup b's column sum of grad_z (the
 *              gradient of the Linear's bias), HGNN_LN_ACT_BLOCKS rows the caller adds (no atomics). */
int hgnn_act_rows_forward_f32(const float* z, int64_t M, int32_t W, int32_t act, float* out, hgnn_stream_t stream);
int hgnn_act_rows_backward_f32(const float* z, const float* grad_out, int64_t M, int32_t W, int32_t act,
                               float* grad_z, float* partials /* [HGNN_LN_ACT_BLOCKS][W] */, hgnn_stream_t stream);

/* ------------------------------------------------------------------------
 * bf16 training path (BASELINE config 4 dtype): backward of the make_mlp Linear layers
 * (Modules/utils.py:169-196 as instantiated at Modules/gnn_utils.py:22-41, :77-115) under the reference's
 * autograd (edge_classifier_base.py:113-128 trains every configuration).
 *
 * hgnn_wgrad_bf16: weight gradient  out[ho, hi] = sum_m A[m, ho] * B[m, hi]  (A = dz [M, Ho], B = the layer's
 *   input rows [M, Hi], both bf16 row-major with row strides lda / ldb in ELEMENTS (multiples of 8, so that a
 *   column slice of a wider matrix can be passed); out fp32 [Ho, ldo]).  Hand-written split-K bf16-MFMA kernel,
 *   fp32 accumulation, partial sums combined in slice order (deterministic, no atomics).  workspace: device
 *   scratch of hgnn_wgrad_workspace_bytes(M, Ho, Hi) bytes.  Ho, Hi multiples of 8.
 * hgnn_ln_act_{forward,backward}_bf16: hgnn_ln_act_*_f32 with bf16 rows (z, grad_out, out / grad_z); fp32
 *   statistics and arithmetic, fp32 gamma / beta / partials.
 */
int hgnn_ln_act_forward_bf16(const void* z, int64_t M, int32_t W, const float* gamma, const float* beta,
                             int32_t act, float eps, void* out, hgnn_stream_t stream);
int hgnn_ln_act_backward_bf16(const void* z, const void* grad_out, int64_t M, int32_t W, const float* gamma,
                              const float* beta, int32_t act, float eps, void* grad_z,
                              float* partials /* [HGNN_LN_ACT_BLOCKS][3][W] */, hgnn_stream_t stream);
int hgnn_wgrad_workspace_bytes(int64_t M, int32_t Ho, int32_t Hi, size_t* bytes);
int hgnn_wgrad_bf16(const void* A, int64_t lda, const void* B, int64_t ldb, int64_t M, int32_t Ho, int32_t Hi,
                    float* out, int64_t ldo, float* colsum /* [Ho] = sum_m A[m, ho] (the bias gradient), or NULL */,
                    void* workspace, size_t workspace_bytes, hgnn_stream_t stream);

/* the same weight gradient for FP32 rows dz [M, Ho] / a [M, Hi] (lda / ldb in floats, multiples of 4, 16-byte aligned
 * rows), the products as split-bf16 (hi.hi + mid.hi + hi.mid, exact products, fp32 accumulation; see
 * hgnn_mlp_forward_f32_split3): the M-row weight-gradient GEMMs of the fp32 training backward.  Workspace as
 * hgnn_wgrad_workspace_bytes. */
int hgnn_wgrad_f32_split3(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t M, int32_t Ho, int32_t Hi,
                          float* out, int64_t ldo, float* colsum, void* workspace, size_t workspace_bytes,
                          hgnn_stream_t stream);

/* hgnn_wgrad_f32: the EXACT weight gradient of the fp32 training backward (additions under ABI 26, as above):
 *   out[ho, hi] = sum_m A[m, ho] * B[m, hi]   with A = dz [M, Ho], B = the layer's input rows [M, Hi], fp32 row-major,
 *   row strides lda / ldb in floats (multiples of 4 that cover the columns; rows 16-byte aligned, so a column slice of
 *   a wider matrix can be passed in place); out fp32 [Ho, ldo], ldo >= Hi.  Ho, Hi: positive multiples of 8, <= 1024.
 *   Every product is formed once from the fp32 operands by v_mfma_f32_16x16x4_f32 (no split, no reduced-precision
 *   plane).  Order contract: split-K over the rows; inside a slice every output element is the chain
 *   acc = fmaf(A[m, ho], B[m, hi], acc) over the slice's rows in order; the slices' partials are added in slice order
 *   by four chains (slices k = 0, 1, 2, 3 mod 4; the remainder joins chain 0) combined as (s0 + s1) + (s2 + s3).  No
 *   atomics.  Slices, rows per slice and tile are a pure function of (M, Ho, Hi) -- never of the device -- so the same
 *   inputs give the same bits on every device and in every run.  M == 0 writes zeros to out and launches nothing else.
 *   No column sums (the fp32 route's bias gradient comes from hgnn_ln_act_backward_f32 / the fp32 backward layer).
 *   workspace: device memory of hgnn_wgrad_f32_workspace_bytes(M, Ho, Hi) bytes, 16-byte aligned.  Every refusal
 *   (HGNN_ERR_INVALID_ARG + hgnn_last_error) is decided before any HIP call and touches no pointer. */
int hgnn_wgrad_f32_workspace_bytes(int64_t M, int32_t Ho, int32_t Hi, size_t* bytes);
int hgnn_wgrad_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t M, int32_t Ho, int32_t Hi,
                   float* out, int64_t ldo, void* workspace, size_t workspace_bytes, hgnn_stream_t stream);

/* The rest of an EXACT fp32 step that used to be library GEMMs (additions under ABI 26, as above): the forward
 * pre-projection and the products with one side at most 32 wide.  For all five entries: every refusal
 * (HGNN_ERR_INVALID_ARG, or HGNN_ERR_UNSUPPORTED for a shape outside the stated ranges, + hgnn_last_error starting with
 * the entry's name) is decided before any HIP call and touches no pointer; no atomics, no scratch memory, no allocation,
 * no host synchronisation; grids, tiles and slices are pure functions of the shape -- never of the device -- so the same
 * inputs give the same bits on every device and in every run.  M <= 2^31 - 1.
 *
 * hgnn_project_f32:  out_b[r, h] = sum_k x[r, k] * w_b[h, k]  for b = 0 and, when w1 / out1 are given (together or not
 *   at all), b = 1: both blocks from ONE launch over the rows of x (the source and destination segment of an edge
 *   update, as hgnn_project_f32_split3).  x [M, K] with row stride ldx; w_b [N, K] row-major with row stride ldw (a
 *   column block W[:, c0:c1] of a first Linear is passed in place); out_b [M, N] with row stride ldo >= N.  All strides
 *   multiples of 4 floats, all rows 16-byte aligned.  K a multiple of 16 in [16, 512], N a multiple of 16 in [16, 1024]
 *   (anything else: HGNN_ERR_UNSUPPORTED).  Order contract: every output element is the chain
 *       acc = 0;  acc = fmaf(x[r, k], w_b[h, k], acc)  for k ASCENDING,
 *   every product formed once on v_mfma_f32_16x16x4_f32 (bitwise a k-ordered fmaf chain); no split-K, hence no
 *   workspace.  One workgroup per (64 rows, block, pass of at most 256 features).  M == 0 launches nothing.
 *
 * The narrow products: n is the narrow width, 1 <= n <= 32; K the wide one, a multiple of 4 in [4, 1024] (anything
 * else: HGNN_ERR_UNSUPPORTED).  fp32 VALU kernels.  Wide-side arrays ([M, K]) need 16-byte aligned rows and strides that
 * are multiples of 4 floats; narrow-side arrays ([M, n], the [n, K] weights and wgrad result, bias, colsum) only 4-byte
 * alignment and any stride that covers their width (tab[N, 3] with 12-byte rows is read in place).
 * hgnn_linear_narrow_f32:  out[m, j] = bias[j] + sum_k x[m, k] * W[j, k]   (bias may be NULL).  Order: a row is shared
 *   by P lanes, P = the largest power of two <= min(K / 4, 64) -- a function of K alone.  Lane t chains
 *   acc = fmaf(x[m, k], W[j, k], acc) from acc = 0 over the k of its 4-float pieces t, t + P, t + 2P, ... ascending; the
 *   P sums are added by a halving tree (v[t] += v[t + h] for h = P/2, P/4, ..., 1); the bias is added last.
 * hgnn_outer_narrow_f32:   out[m, k] = sum_j y[m, j] * W[j, k] (+ add[m, k]).  Order: acc = 0; acc = fmaf(y[m, j],
 *   W[j, k], acc) for j ascending from 0; add (NULL or [M, K] with out's row stride ldo) joins last with one rounding.
 * hgnn_wgrad_narrow_f32:   out[j, k] = sum_m y[m, j] * x[m, k];  colsum[j] = sum_m y[m, j] (optional: a head's bias
 *   gradient).  Order: the rows are split into S slices of L rows, with ng = ceil(n / 8) and
 *       want = clamp(ceil(131072 / ((K / 4) * ng)), 1, max(1, ceil(M / 64))),  L = max(16, 16 * ceil(ceil(M / want) / 16)),
 *       S = ceil(max(M, 1) / L);
 *   inside a slice every element is the chain acc = fmaf(y[m, j], x[m, k], acc) (colsum: acc += y[m, j]) from acc = 0
 *   over the slice's rows in order; the slices are added in hgnn_wgrad_f32's four-chain order, (s0 + s1) + (s2 + s3)
 *   with the remainder on chain 0.  workspace: hgnn_wgrad_narrow_f32_workspace_bytes(M, n, K) = S * n * (K + 1) floats
 *   of device memory, 4-byte aligned.  M == 0 writes zeros to out (and colsum). */
int hgnn_project_f32(const float* x, int64_t ldx, int64_t M, int32_t K, const float* w0, const float* w1, int64_t ldw,
                     int32_t N, float* out0, float* out1, int64_t ldo, hgnn_stream_t stream);
int hgnn_linear_narrow_f32(const float* x, int64_t ldx, int64_t M, int32_t K, const float* W, int64_t ldw,
                           const float* bias, int32_t n, float* out, int64_t ldo, hgnn_stream_t stream);
int hgnn_outer_narrow_f32(const float* y, int64_t ldy, int64_t M, int32_t n, const float* W, int64_t ldw, int32_t K,
                          const float* add, float* out, int64_t ldo, hgnn_stream_t stream);
int hgnn_wgrad_narrow_f32_workspace_bytes(int64_t M, int32_t n, int32_t K, size_t* bytes);
int hgnn_wgrad_narrow_f32(const float* y, int64_t ldy, int32_t n, const float* x, int64_t ldx, int32_t K, int64_t M,
                          float* out, int64_t ldo, float* colsum, void* workspace, size_t workspace_bytes,
                          hgnn_stream_t stream);

/* hgnn_mlp_backward_layer_bf16: the hand-written DATA gradient of one Linear of the bf16 training path, fused with
 * what follows it in the backward:
 *   z_prev != NULL ("LayerNorm form"):  da = dz[M,K] . W[K,N];  out = dz' = dLayerNorm(act'(LN(z_prev)) * da)  with
 *       z_prev [M,N] the previous layer's pre-LayerNorm rows (bf16 dumps of the forward), ln_w / ln_b / act / eps that
 *       layer's LayerNorm + activation; a_prev (optional) receives act(LN(z_prev)) (the rows hgnn_wgrad_bf16 needs
 *       for W's gradient); partials: float [HGNN_MLP_BWD_BLOCKS][2][N] per-workgroup column sums of dgamma / dbeta
 *       (the caller adds them; the bias gradient = column sums of dz' comes from hgnn_wgrad_bf16's colsum);
 *   z_prev == NULL ("input form"):      out = dz . W (+ skip): gradient of a direct input segment of the first
 *       layer, the skip connection's gradient (skip [M,N] bf16, may be NULL) added in the epilogue.
 * Wt_frag: W^T (the [N][K] matrix) in the MFMA A-fragment order of hgnn_mlp_forward_bf16_split.
 * K a multiple of 128, N in {128, 256, 512, 1024}; all rows bf16, fp32 accumulation and LayerNorm arithmetic;
 * deterministic.  A workgroup walks row tiles of 64 rows (N <= 512) or HGNN_MLP_BWD_TILE_ROWS_N1024 rows (N = 1024,
 * the hidden width of latent 512: 8 waves, 8 feature tiles each). */
#define HGNN_MLP_BWD_BLOCKS 512
#define HGNN_MLP_BWD_TILE_ROWS_N1024 32
int hgnn_mlp_backward_layer_supported_bf16(int32_t K, int32_t N);
int hgnn_mlp_backward_layer_bf16(const void* dz, int64_t M, int32_t K, int32_t N, const void* Wt_frag,
                                 const void* z_prev, const float* ln_w, const float* ln_b, int32_t act, float eps,
                                 const void* skip, void* out, void* a_prev, float* partials, hgnn_stream_t stream);

/* hgnn_mlp_backward_layer_f32: the same fused backward layer for the EXACT fp32 training path, fp32 rows throughout, on
 * the fp32 matrix instruction (v_mfma_f32_16x16x4_f32: a chain of fused multiply-adds, as hgnn_mlp_forward_f32):
 *   z_prev != NULL ("LayerNorm form"):  da = dz[M,K] . W[K,N];  out = dz' = dLayerNorm(act'(LN(z_prev)) * da);  a_prev
 *       (optional) receives act(LN(z_prev)); partials: float [HGNN_MLP_BWD_F32_BLOCKS][3][N] per-workgroup column sums
 *       of dgamma, dbeta and dz' (the previous Linear's bias gradient) -- the three sums of hgnn_ln_act_backward_f32;
 *       the caller adds the partial rows, idle workgroups write zeros.  ln_w, ln_b and partials are required, skip
 *       must be NULL.  M = 0 writes zero partials.
 *   z_prev == NULL ("input form"):      out = dz . W (+ skip), skip [M,N] or NULL; a_prev and partials must be NULL.
 * Wt: W^T, i.e. the [N][K] matrix Wt[n][k] = W[k][n], plain row-major fp32 (row stride K).  dz [M,K], z_prev / skip /
 * out / a_prev [M,N] row-major; every pointer 16-byte aligned.  K a multiple of 16 with 64 <= K <= 1024, N in
 * {64, 128, 256, 512} (anything else: HGNN_ERR_UNSUPPORTED, nothing written); act = HGNN_ACT_*, exact-erf GELU.
 * LayerNorm statistics are centred (mean first, then sum((z - mean)^2)).  One wave owns 16 rows and all N features;
 * workgroups walk the 64-row tiles in a fixed order on a grid that does not depend on the device, the column sums are
 * combined in a fixed order without atomics: the same inputs give the same bits everywhere. */
#define HGNN_MLP_BWD_F32_BLOCKS 512
int hgnn_mlp_backward_layer_supported_f32(int32_t K, int32_t N);
int hgnn_mlp_backward_layer_f32(const float* dz, int64_t M, int32_t K, int32_t N, const float* Wt,
                                const float* z_prev, const float* ln_w, const float* ln_b, int32_t act, float eps,
                                const float* skip, float* out, float* a_prev,
                                float* partials /* [HGNN_MLP_BWD_F32_BLOCKS][3][N] */, hgnn_stream_t stream);

/* ------------------------------------------------------------------------
 * Tracking-performance metrics (reference Modules/tracking_utils.py:18-83, eval_metrics, cupy / cupy.sparse
 * there; the validation and test steps of every training base end in it).  ABI 25.
 *
 * hgnn_track_eval: pairs (hit[b], cand[b]), b < n_pairs, assign hits to track candidates (int64 labels, any
 *   values); the event's truth is pid[n_hits] (int64, 0 = noise), pt[n_hits] (float32) and, or NULL,
 *   primary[n_hits] (uint8, != 0 = primary; NULL = primary=False in the reference).  Candidates with
 *   float(count) < float(nhits_cut * majority_cut) pairs are dropped, the rest relabelled densely; particles are
 *   the distinct pids.  The matching, its filter and the four metrics follow the reference exactly (DESIGN.md
 *   section 3, "Tracking metrics").  majority_cut > 0.  result: device double[HGNN_TE_RESULT] (indices below).
 *   A hit id outside [0, n_hits) does not fault: result[HGNN_TE_STATUS] = 1 and the other entries are
 *   meaningless.  No match before or after the filter (also: no pair survives the size filter) gives
 *   result[HGNN_TE_NO_MATCH] = 1, the reference's default_response.  Deterministic: two calls give the same bits.
 * hgnn_track_eval_workspace_bytes: device scratch of one call (any 256-B aligned).
 * ------------------------------------------------------------------------ */
#define HGNN_TE_TRACK_EFF 0
#define HGNN_TE_TRACK_PUR 1
#define HGNN_TE_HIT_EFF 2
#define HGNN_TE_HIT_PUR 3
#define HGNN_TE_N_KEPT 4    /* matches kept by the filter (n > majority_cut * nhits_cut, pid != 0) */
#define HGNN_TE_N_MASK 5    /* kept matches of reconstructable particles                           */
#define HGNN_TE_N_TRUTH 6   /* reconstructable particles                                           */
#define HGNN_TE_N_CAND 7    /* C: candidates after the size filter                                 */
#define HGNN_TE_N_PART 8    /* P: distinct pids                                                    */
#define HGNN_TE_NO_MATCH 9  /* 1: default_response                                                 */
#define HGNN_TE_STATUS 10   /* 1: a hit id was out of range                                        */
#define HGNN_TE_N_MATCH 11  /* matches before the filter                                           */
#define HGNN_TE_RESULT 12
int hgnn_track_eval_workspace_bytes(int64_t n_pairs, int64_t n_hits, size_t* bytes);
int hgnn_track_eval(const int64_t* hit, const int64_t* cand, int64_t n_pairs, const int64_t* pid, const float* pt,
                    const uint8_t* primary, int64_t n_hits, double pt_cut, double nhits_cut, double majority_cut,
                    double* result, void* workspace, size_t workspace_bytes, hgnn_stream_t stream);

/* hgnn_track_records: hgnn_track_eval's pipeline (the same sorts, contingency triples and match rule), keeping
 *   what that entry folds into its 12 doubles.  Added under ABI 26: additions only.  The arguments shared with
 *   hgnn_track_eval mean the same, and result[HGNN_TE_*] has the same bits for the same inputs.
 *   Particle table (struct hgnn_tr_particles, device arrays of n_hits rows; rows p < P = result[HGNN_TE_N_PART]
 *   are written, in ascending pid; the other rows are unspecified): pid; nhits; pt, the minimum over the
 *   particle's hits in which a NaN wins (and -0.0 is below 0.0, so the bits do not depend on the order); primary (any hit primary; 0 with primary == NULL); reconstructable
 *   (pt > float(pt_cut), nhits >= nhits_cut and, with primary, primary: the particles HGNN_TE_N_TRUTH counts, the
 *   noise particle pid 0 included as there); n_match / n_kept / n_mask, the particle's matches before the filter,
 *   kept by it, and kept and reconstructable; cand_index, the SMALLEST dense candidate index among its kept
 *   matches, or -1, and shared, that triple's pair count n, or 0 (a particle can keep two matches: for C above
 *   about 4500 neighbouring hash values round to the same double); values [n_vars][n_hits], every binning variable
 *   reduced over the particle's hits exactly as pt is.
 *   Candidate table (struct hgnn_tr_candidates, device arrays of n_pairs rows; rows c < C = result[HGNN_TE_N_CAND]
 *   are written, in ascending label): label, the original label; size, its pairs (duplicates counted); n_kept /
 *   n_mask, the kept and the masked matches that name it; particle, the SMALLEST particle row among its kept
 *   matches, or -1, and shared, that triple's n, or 0 (with majority_cut <= 0.5 two particles can hold one
 *   candidate).
 *   Binning: vars is device float32 [n_vars][n_hits] (NULL with n_vars == 0), 0 <= n_vars <= HGNN_TR_MAX_VARS.
 *   edges (float32 [n_vars][HGNN_TR_MAX_BINS + 1]) and n_bins (int32 [n_vars], each in [1, HGNN_TR_MAX_BINS])
 *   are HOST arrays, read before the call returns; the first n_bins[v] + 1 edges of row v are used and must be
 *   finite and strictly ascending.  The slot of particle p for variable v is the number of edges <= values[v][p],
 *   compared in float32 (numpy.searchsorted(edges, x, side="right")): slot 0 is the underflow, 1 .. nb the bins,
 *   nb + 1 the overflow, where a NaN lands too.  hist is device int64 [n_vars][HGNN_TR_MAX_BINS + 2]
 *   [HGNN_TR_COLUMNS] (slots above nb + 1 stay 0); the columns of a slot: particles, reconstructable particles,
 *   sum of n_kept, sum of n_mask, sum of n over the masked triples, sum of nhits * n_mask.  Over all slots the
 *   first four add up to HGNN_TE_N_PART, N_TRUTH, N_KEPT and N_MASK (with n_pairs == 0 result[] is the default
 *   response and says N_TRUTH = 0, while the particle table and the first two columns are still filled).
 *   A hit id outside [0, n_hits) does not fault: result[HGNN_TE_STATUS] = 1 and everything else is meaningless.
 *   Integer counting only (integer atomics on the candidate side and in the histogram): two calls give the same
 *   bits.  Allocates nothing; launches on `stream`.
 * hgnn_track_records_workspace_bytes: device scratch of one call (any 256-B aligned). */
#define HGNN_TR_MAX_VARS 4
#define HGNN_TR_MAX_BINS 64
#define HGNN_TR_COLUMNS 6
struct hgnn_tr_particles {
    int64_t* pid;
    int32_t* nhits;
    float* pt;
    uint8_t* primary;
    uint8_t* reconstructable;
    int32_t* n_match;
    int32_t* n_kept;
    int32_t* n_mask;
    int32_t* cand_index;
    int32_t* shared;
    float* values; /* [n_vars][n_hits]; NULL with n_vars == 0 */
};
struct hgnn_tr_candidates {
    int64_t* label;
    int32_t* size;
    int32_t* n_kept;
    int32_t* n_mask;
    int32_t* particle;
    int32_t* shared;
};
int hgnn_track_records_workspace_bytes(int64_t n_pairs, int64_t n_hits, int32_t n_vars, size_t* bytes);
int hgnn_track_records(const int64_t* hit, const int64_t* cand, int64_t n_pairs, const int64_t* pid, const float* pt,
                       const uint8_t* primary, int64_t n_hits, const float* vars, int32_t n_vars, const float* edges,
                       const int32_t* n_bins, double pt_cut, double nhits_cut, double majority_cut, double* result,
                       const struct hgnn_tr_particles* particles, const struct hgnn_tr_candidates* candidates,
                       int64_t* hist, void* workspace, size_t workspace_bytes, hgnn_stream_t stream);

/* hgnn_track_scan: the tracking metrics of ONE event at n_cuts score cuts, in one call.  Added under ABI 26: additions only.
 *   mode HGNN_TS_EDGE: a = src, b = dst (int64 [n_items]) are the edges of a graph on n_vertices vertices; the
 *   candidates at a cut are the weakly connected components of the edges with score >= cut, and the evaluated pairs
 *   are (inverse_mask[v], smallest vertex id of v's component) over the vertices v that touch such an edge
 *   (hgnn_cc_labels at that cut; an edge with a vertex id outside [0, n_vertices) is skipped).  When no edge passes a
 *   cut, the components of all edges with a non-NaN score are taken instead (edge_classifier_base.py:157-168).
 *   mode HGNN_TS_PAIR: a = hit, b = cand (int64 [n_items]); the evaluated pairs at a cut are those with
 *   score >= cut, hit ids mapped through inverse_mask (int64 [n_vertices]) when it is not NULL; with a mask, a hit
 *   id outside [0, n_vertices) of a passing pair sets the status.  The label HGNN_TS_RESERVED_LABEL is reserved.
 *   Every comparison is score >= cut in float32: a NaN score passes no cut.
 *   cuts: DEVICE float32 [n_cuts], 1 <= n_cuts <= HGNN_TS_MAX_CUTS, in any order, repeats allowed, none NaN (the
 *   rows of a list with a NaN cut are unspecified; nothing faults).
 *   result: device double [n_cuts][HGNN_TS_ROW], row t for cuts[t].  Entries 0 .. HGNN_TE_RESULT - 1 are bit for bit
 *   what hgnn_track_eval writes for that pair set (a cut with no pair: its n_pairs == 0 row), with
 *   result[HGNN_TE_STATUS] = 2 when a passing pair carries the reserved label (that row is meaningless).  With truth
 *   (uint8 [n_items]) the last three entries count items, keep (uint8 [n_items], NULL = all) selecting them:
 *   N_PASS = #{keep, score >= cut}, N_TRUE_PASS = #{keep, truth, score >= cut}, N_TRUE = #{keep, truth}; without
 *   truth they are 0.  pid, pt, primary, n_hits, pt_cut, nhits_cut, majority_cut: as for hgnn_track_eval.
 *   Integer counting and the fixed-order sums of hgnn_track_eval only: two calls give the same bits.  Allocates
 *   nothing; launches on `stream`; reads nothing back.
 * hgnn_track_scan_workspace_bytes: device scratch of one call (any 256-B aligned). */
#define HGNN_TS_EDGE 0
#define HGNN_TS_PAIR 1
#define HGNN_TS_MAX_CUTS 64
#define HGNN_TS_N_PASS 12
#define HGNN_TS_N_TRUE_PASS 13
#define HGNN_TS_N_TRUE 14
#define HGNN_TS_ROW 15
#define HGNN_TS_RESERVED_LABEL INT64_MAX
int hgnn_track_scan_workspace_bytes(int32_t mode, int64_t n_items, int64_t n_vertices, int64_t n_hits, int32_t n_cuts,
                                    size_t* bytes);
int hgnn_track_scan(int32_t mode, const int64_t* a, const int64_t* b, int64_t n_items, const float* score,
                    const float* cuts, int32_t n_cuts, const int64_t* inverse_mask, int64_t n_vertices,
                    const uint8_t* truth, const uint8_t* keep, const int64_t* pid, const float* pt,
                    const uint8_t* primary, int64_t n_hits, double pt_cut, double nhits_cut, double majority_cut,
                    double* result, void* workspace, size_t workspace_bytes, hgnn_stream_t stream);

/* ------------------------------------------------------------------------
 * graph_intersection of the embedding stage (reference Modules/utils.py:117-166, scipy CSR there).  ABI 26.
 *
 * hgnn_graph_intersection: pred [2, e_pred] and truth [2, e_truth] int64 (rows, then cols), ids in [0, 2^31).
 *   out_graph [2, e_pred] int64 (row stride e_pred) receives the U distinct pred pairs in row-major order,
 *   out_y [e_pred] uint8 whether each also occurs in truth; with weights (truth's, float32 or float64 by
 *   weight_dtype = HGNN_DT_F32 / HGNN_DT_F64; NULL = no weights, out_weights NULL too) out_weights [e_pred] of that
 *   dtype receives the sum of the weights over the truth copies of each output pair (0 if none), summed in the
 *   truth order.  out_count_and_status: device int64[2] = {U, status}; status 1 = an id outside [0, 2^31) (nothing
 *   else is written, never a fault).  Only out[.., :U] is meaningful.  Allocates nothing, never synchronises;
 *   deterministic.
 * hgnn_graph_intersection_workspace_bytes: device scratch of one call (any 256-B aligned).
 * ------------------------------------------------------------------------ */
int hgnn_graph_intersection_workspace_bytes(int64_t e_pred, int64_t e_truth, int32_t with_weights, size_t* bytes);
int hgnn_graph_intersection(const int64_t* pred, int64_t e_pred, const int64_t* truth, int64_t e_truth,
                            const void* weights, int32_t weight_dtype, int64_t* out_graph, uint8_t* out_y,
                            void* out_weights, int64_t* out_count_and_status, void* workspace,
                            size_t workspace_bytes, hgnn_stream_t stream);

/* ------------------------------------------------------------------------
 * Max-weight bipartite matching of the assignment loss (reference BipartiteClassification/
 * bipartite_classification_base.py:152-191 and gmrt_base.py:159-198; scipy CSR and
 * min_weight_full_bipartite_matching on the host there).  Added under ABI 26.
 *
 * hgnn_assign_match: edges (row[b], col[b], score[b]), b < n_edges, row in [0, n_rows), col in [0, n_cols), score
 *   float32.  pair_row / pair_col / pair_weight [n_edges] receive the U distinct (row, col) pairs in row-major order
 *   and, in float64, the sum of each pair's scores in ascending original position.  col_match [n_rows]: every row is
 *   matched to one real column among its pairs, no column twice, or to its private virtual column n_cols + row
 *   (weight HGNN_AM_FALLBACK_WEIGHT), so that the total weight is maximal for the weights rint(w * 2^S), S =
 *   HGNN_AM_SCALE_BITS: at most (n_rows + n_cols) * 2^-S below the optimum of the float64 weights, and exactly
 *   optimal when every weight is a multiple of 2^-S.  Pairs whose weight rounds to 0 tie with the virtual column.
 *   Solved by an integer eps-scaled auction on the device (csrc/assign.hip); deterministic.
 *   info: HOST int64[HGNN_AM_INFO] (indices below).  info[HGNN_AM_STATUS] != 0 (HGNN_AM_ST_* bits): col_match is
 *   not written; the return value is still HGNN_OK.  Nothing faults on a bad id.
 *   Unlike the other entry points this one SYNCHRONISES the stream: it reads a few words back once after the
 *   contraction and once per tail launch, info[HGNN_AM_HOST_READS] <= 48 times in all (it gives up with
 *   HGNN_AM_ST_BUDGET before it would exceed that), so it cannot be captured into a graph.  It allocates nothing.
 *   Every device loop has a round budget; there is no grid-wide barrier.
 * hgnn_assign_match_workspace_bytes: device scratch of one call (any 256-B aligned).
 * ------------------------------------------------------------------------ */
#define HGNN_AM_SCALE_BITS 30
#define HGNN_AM_FALLBACK_WEIGHT 1e-12
#define HGNN_AM_ST_BAD_ID 1      /* a row or col id out of range                                     */
#define HGNN_AM_ST_BAD_WEIGHT 2  /* a pair weight is not finite or |rint(w * 2^S)| * (n + 1) > 2^56  */
#define HGNN_AM_ST_OVERFLOW 4    /* a price left the guarded int64 range                             */
#define HGNN_AM_ST_BUDGET 8      /* the round / host-read budget ran out                             */
#define HGNN_AM_N_PAIRS 0
#define HGNN_AM_STATUS 1
#define HGNN_AM_PHASES 2
#define HGNN_AM_GRID_ROUNDS 3    /* rounds run as grid launches (idle ones included) */
#define HGNN_AM_TAIL_ROUNDS 4    /* rounds run inside the single-workgroup kernel    */
#define HGNN_AM_HOST_READS 5
#define HGNN_AM_INFO 8
int hgnn_assign_match_workspace_bytes(int64_t n_edges, int64_t n_rows, int64_t n_cols, size_t* bytes);
int hgnn_assign_match(const int64_t* row, const int64_t* col, const float* score, int64_t n_edges, int64_t n_rows,
                      int64_t n_cols, int64_t* col_match, int64_t* pair_row, int64_t* pair_col, double* pair_weight,
                      int64_t* info, void* workspace, size_t workspace_bytes, hgnn_stream_t stream);

/* ------------------------------------------------------------------------
 * Deterministic HDBSCAN* (reference GNNEmbedding/embedding_base.py:40-41,267-272: cuml.cluster.HDBSCAN with
 * metric='euclidean', cluster_selection_method='eom').  Added under ABI 26: additions only.
 *
 * hgnn_hdbscan_f32: points float32 [N, D] (row-major, D <= 16, N <= 2^21).  Definition (DESIGN.md section 3,
 *   "HDBSCAN"; alpha = 1, cluster_selection_epsilon = 0, no single-cluster result):
 *     core2[i]  = the min_samples-th smallest squared distance from i, i itself counted (min_samples <= 128);
 *     w2(i, j)  = max(core2[i], core2[j], d2(i, j)), d2 = the float32 sum of the squared float32 differences in
 *                 dimension order (one rounded product and one rounded sum per dimension);
 *     the UNIQUE minimum spanning tree under the strict total order (w2, min(i, j), max(i, j));
 *     all tree edges of equal w2 are one simultaneous multi-way merge; read top-down a level is a true split iff at
 *     least two of its parts hold >= min_cluster_size points (the smaller parts fall out of the parent there),
 *     otherwise the parts below min_cluster_size fall out of the continuing cluster;
 *     lambda = 1 / sqrt(w2) in float64 (HGNN_HDBSCAN_LAMBDA_DUP for w2 = 0, duplicate points), float64 stabilities,
 *     EOM: a cluster is selected iff its stability >= the sum of the selected stabilities below it; never the root.
 *   No tie is broken by arrival order: the partition does not depend on the order of the points.
 *   Outputs (device): labels int64 [N] (-1 noise; clusters 0..C-1 by smallest member index), mst_edges int64
 *   [N-1, 2] (min id first) and mst_w2 float32 [N-1] sorted by (w2, min, max), core2 float32 [N].
 *   info: HOST int64[HGNN_HDB_INFO] or NULL (indices below).  On entry info[HGNN_HDB_STAGE_SYNC] != 0 asks for two
 *   extra stream synchronisations so that the core-distance and sort stages are timed on their own (measurement
 *   tools); otherwise the first round's time includes the core distances.  Times are host-clock nanoseconds.
 *   Like hgnn_assign_match this entry SYNCHRONISES the stream: one read of the edge count per Boruvka round
 *   (<= 21 rounds), one device-to-host copy of the sorted edges and one host-to-device copy of the labels around
 *   the sequential tree stage, which is host code; info[HGNN_HDB_HOST_READS] <= 24.  It cannot be captured into a
 *   graph.  Non-finite coordinates end in HGNN_ERR_INVALID_ARG (a round joins nothing), never in a fault.
 * hgnn_hdbscan_workspace_bytes: device scratch of one call (any 256-B aligned).
 * hgnn_hdbscan_tree_host: the tree stage alone, host pointers only (no device is touched): edges int64 [N-1, 2] of
 *   a spanning tree with w2 [N-1] ascending -> labels [N], *n_clusters (may be NULL).
 * ------------------------------------------------------------------------ */
#define HGNN_HDBSCAN_LAMBDA_DUP 0x1p100 /* above 1 / sqrt(smallest positive float32) = 2.7e22 */
#define HGNN_HDB_ROUNDS 0
#define HGNN_HDB_HOST_READS 1
#define HGNN_HDB_N_CLUSTERS 2
#define HGNN_HDB_STAGE_SYNC 3
#define HGNN_HDB_T_CORE_NS 4
#define HGNN_HDB_T_SORT_NS 5   /* sort, edge emission and the copy of the edges to the host */
#define HGNN_HDB_T_TREE_NS 6   /* the host tree stage alone                                  */
#define HGNN_HDB_T_ROUND0_NS 8 /* .. + round                                                 */
#define HGNN_HDB_INFO 32
int hgnn_hdbscan_workspace_bytes(int64_t N, int32_t D, int32_t min_cluster_size, int32_t min_samples, size_t* bytes);
int hgnn_hdbscan_f32(const float* points, int64_t N, int32_t D, int32_t min_cluster_size, int32_t min_samples,
                     int64_t* labels, int64_t* mst_edges, float* mst_w2, float* core2, int64_t* info, void* workspace,
                     size_t workspace_bytes, hgnn_stream_t stream);
int hgnn_hdbscan_tree_host(const int64_t* edges, const float* w2, int64_t N, int32_t min_cluster_size,
                           int64_t* labels, int64_t* n_clusters);

/* ------------------------------------------------------------------------
 * Weighted squared pair hinge loss of the embedding stage (reference GNNEmbedding/embedding_base.py:95-107,
 * :137-155, :167-168: pt_weighting + get_training_weight + get_hinge_distance + hinge_embedding_loss(..)^2 . weights,
 * a few dozen elementwise library kernels and several host reads there).  Added under ABI 26: additions only.
 *
 * E float32 [N, D] (1 <= D <= HGNN_PH_MAX_DIM), graph [2, P] pair ids (row a, then row b; int32 or int64 by
 * index_dtype = HGNN_DT_I32 / HGNN_DT_I64), y uint8 [P] (!= 0 = true pair), pt float32 [N]; hparams: HOST
 * double[HGNN_PH_HPARAMS] (indices below), read before the call returns.  Definition ("k_ph"):
 *     ptw(p) = pt_weighting(p), NaN read as 0, in float32;   raw_i = ptw(pt[a_i]) + ptw(pt[b_i])
 *     S_T = sum_{y_i} raw_i,  S_F = sum_{!y_i} raw_i
 *     w_i = raw_i / S_T * sigmoid(lwr) if y_i, else raw_i / S_F * sigmoid(-lwr)
 *     d_i = sqrt(|E[a_i] - E[b_i]|^2 + 1e-12) (float32),  l_i = y_i ? scale d_i : max(0, margin - scale d_i)
 *     loss = sum_i w_i l_i^2
 *   A class whose weights sum to 0 -- an empty class in particular -- contributes nothing (the reference divides 0 by
 *   0 there and returns NaN); P = 0 gives 0.  S_T, S_F and the loss are float64 sums in a fixed order that depends on
 *   P alone: two calls give the same bits, and a permutation of the pairs changes the loss by float64 rounding only.
 * hgnn_pair_hinge_forward: loss device float[1]; state device double[HGNN_PH_STATE] (what the backward needs, and the
 *   loss and the class sums in float64); status device int32[1], cleared first: 1 = an endpoint outside [0, N) (such
 *   pairs are skipped, never a fault).
 * hgnn_pair_hinge_backward: grad_E [N, D] (every element written) = grad_out[0] * d loss / d E, the only gradient;
 *   grad_out device float[1]; state as the forward wrote it; plan: the built gather plan with dst_index = cat(a, b),
 *   gather_index = cat(b, a) (int64 [2P]), n_dst = n_src = N -- it may be built before the forward and reused.  Each
 *   row is the sum of its list in the plan's order (stable by position), formed as c_i (E[v] - E[other]): no atomics,
 *   the same bits for every launch shape and plan chunk.
 * Both launch asynchronously, allocate nothing and never synchronise.
 * hgnn_pair_hinge_workspace_bytes: device scratch of one forward (backward = 0) or backward (1) call (256-B aligned).
 * ------------------------------------------------------------------------ */
#define HGNN_PH_MAX_DIM 16
#define HGNN_PH_WEIGHT_MIN 0
#define HGNN_PH_WEIGHT_LEAK 1
#define HGNN_PH_PTCUT 2
#define HGNN_PH_PT_INTERVAL 3
#define HGNN_PH_LOG_WEIGHT_RATIO 4
#define HGNN_PH_MARGIN 5
#define HGNN_PH_SCALE 6
#define HGNN_PH_HPARAMS 8
#define HGNN_PH_KT 0     /* sigmoid(lwr) / S_T, 0 for a class without weight */
#define HGNN_PH_KF 1     /* sigmoid(-lwr) / S_F                               */
#define HGNN_PH_ST 2
#define HGNN_PH_SF 3
#define HGNN_PH_LOSS 4   /* the loss before it is rounded to float32          */
#define HGNN_PH_STATE 8
int hgnn_pair_hinge_workspace_bytes(int64_t P, int64_t N, int32_t D, int32_t backward, size_t* bytes);
int hgnn_pair_hinge_forward(const float* E, int64_t N, int32_t D, const void* graph, int32_t index_dtype,
                            const uint8_t* y, const float* pt, int64_t P, const double* hparams, float* loss,
                            double* state, int32_t* status, void* workspace, size_t workspace_bytes,
                            hgnn_stream_t stream);
int hgnn_pair_hinge_backward(const hgnn_plan* plan, const float* E, int64_t N, int32_t D, const void* graph,
                             int32_t index_dtype, const uint8_t* y, const float* pt, int64_t P, const double* hparams,
                             const double* state, const float* grad_out, float* grad_E, void* workspace,
                             size_t workspace_bytes, hgnn_stream_t stream);

/* ------------------------------------------------------------------------
 * pT-weighted binary cross-entropy: the edge classifier's loss (reference EdgeClassifier/edge_classifier_base.py
 * :99-111, :127-128) and the assignment loss after the matching (bipartite_classification_base.py:123-138, :189-190)
 * as one operator.  Added under ABI 26: additions only.
 *
 * scores float32 [P] in [0, 1]; graph [2, P] pair ids (row a in [0, NA), then row b in [0, NB); int32 or int64 by
 * index_dtype); y uint8 [P] (!= 0 = true pair); keep uint8 [P] or NULL (NULL = every pair; a pair with keep == 0
 * contributes to nothing); pt_a float32 [NA], pt_b float32 [NB] (the same pointer for one table); combine =
 * HGNN_WB_COMBINE_SUM (edge classifier) or HGNN_WB_COMBINE_MAX (assignment); hparams: HOST double[HGNN_PH_HPARAMS],
 * entries HGNN_PH_WEIGHT_MIN .. HGNN_PH_LOG_WEIGHT_RATIO (0-4) are read, before the call returns.  Definition
 * ("k_wb"), ptw as for the pair hinge:
 *     raw_i = combine(ptw(pt_a[a_i]), ptw(pt_b[b_i])),  S_T = sum_{keep, y} raw_i,  S_F = sum_{keep, !y} raw_i
 *     l_i = -(y_i ? max(log(s_i), -100) : max(log(1 - s_i), -100))   (float32, 1 - s_i formed in float32)
 *     loss = sigmoid(lwr) / S_T * sum_{keep, y} raw_i l_i + sigmoid(-lwr) / S_F * sum_{keep, !y} raw_i l_i
 *   A class whose weights sum to 0 contributes nothing (the reference's 0/0 is NaN); P = 0 gives 0.  The four sums
 *   are float64 sums in a fixed order that depends on P alone: two calls give the same bits.
 * hgnn_weighted_bce_forward: loss device float[1]; state device double[HGNN_WB_STATE] (indices below); status device
 *   int32[1], cleared first, then the OR of HGNN_WB_ST_BAD_ID (an id out of range) and HGNN_WB_ST_BAD_SCORE (a score
 *   that is NaN or outside [0, 1]); such pairs are skipped like dropped ones, never a fault.
 * hgnn_weighted_bce_backward: grad_scores float32 [P], every element written:
 *     grad_out[0] * k_class(i) * raw_i * (s_i - y_i) / max((1 - s_i) * s_i, 1e-12),  0 for a dropped or skipped pair;
 *   grad_out device float[1]; state as the forward wrote it.  No atomics, no workspace.
 * Both launch asynchronously, allocate nothing and never synchronise.
 * hgnn_weighted_bce_workspace_bytes: device scratch of one forward (backward = 0) or backward (1) call.
 * ------------------------------------------------------------------------ */
#define HGNN_WB_COMBINE_SUM 0
#define HGNN_WB_COMBINE_MAX 1
#define HGNN_WB_ST_BAD_ID 1
#define HGNN_WB_ST_BAD_SCORE 2
#define HGNN_WB_KT 0     /* sigmoid(lwr) / S_T, 0 for a class without weight */
#define HGNN_WB_KF 1     /* sigmoid(-lwr) / S_F                               */
#define HGNN_WB_ST 2
#define HGNN_WB_SF 3
#define HGNN_WB_LOSS 4   /* the loss before it is rounded to float32          */
#define HGNN_WB_STATE 8
int hgnn_weighted_bce_workspace_bytes(int64_t P, int32_t backward, size_t* bytes);
int hgnn_weighted_bce_forward(const float* scores, const void* graph, int32_t index_dtype, const uint8_t* y,
                              const uint8_t* keep, const float* pt_a, int64_t NA, const float* pt_b, int64_t NB,
                              int64_t P, int32_t combine, const double* hparams, float* loss, double* state,
                              int32_t* status, void* workspace, size_t workspace_bytes, hgnn_stream_t stream);
int hgnn_weighted_bce_backward(const float* scores, const void* graph, int32_t index_dtype, const uint8_t* y,
                               const uint8_t* keep, const float* pt_a, int64_t NA, const float* pt_b, int64_t NB,
                               int64_t P, int32_t combine, const double* hparams, const double* state,
                               const float* grad_out, float* grad_scores, hgnn_stream_t stream);

/* ------------------------------------------------------------------------
 * The optimiser step of the training bases as one operator: clip_grad_norm_(max_norm) over all gradients, then
 * torch.optim.AdamW (decoupled weight decay, amsgrad or not), then optionally zero_grad (reference
 * Modules/.../..._base.py configure_optimizers, Trainer(gradient_clip_val)).  Added under ABI 26: additions only.
 *
 * The tensors of one step are described by a table of hgnn_opt_entry, one per parameter that has a gradient, given
 * twice: host_table (HOST memory, read and checked before the call returns) and table (the same bytes in DEVICE
 * memory, read by the kernels).  p and g are float32 device arrays of numel elements, 4-byte aligned; the tensor's
 * exp_avg, exp_avg_sq and max_exp_avg_sq are the elements [offset, offset + numel) of three flat float32 buffers of
 * state_numel elements each.  The work is cut into chunks of HGNN_OPT_CHUNK consecutive elements of one tensor;
 * first_chunk is the number of chunks of the entries before this one (entry i owns ceil(numel_i / HGNN_OPT_CHUNK)
 * chunks) and n_chunks their total.  Tensors whose p, g and offset are 16-byte aligned are moved in 16-byte words,
 * others and tails element by element; both give the same bits.  The scalars are this step's, per tensor, rounded
 * from double:
 *     decay = 1 - lr wd, step_size = lr / (1 - b1^t), inv_sqrt_bc2 = 1 / sqrt(1 - b2^t), one_minus_b1, b2,
 *     one_minus_b2, eps
 * Per element, float32, every operation rounded on its own ("k_opt"):
 *     g' = g coef;  p *= decay;  m += (g' - m) one_minus_b1;  v = v b2 + (one_minus_b2 g') g';  vmax = max(vmax, v);
 *     p -= step_size (m / (sqrt(vmax) inv_sqrt_bc2 + eps))            (v for vmax without HGNN_OPT_AMSGRAD)
 * hgnn_optim_grad_norm: state device double[HGNN_OPT_STATE]: total_norm = sqrt(sum g^2) (a float64 sum in a fixed
 *   order that depends on the tensor sizes alone: two calls give the same bits), coef = min(1, max_norm /
 *   (total_norm + 1e-6)) formed in float32 (NaN stays NaN), and the sum.  status device int32[1]: HGNN_OPT_ST_NONFINITE
 *   is OR-ed into it when total_norm is inf or NaN; the call never clears it.  flags: 0 or HGNN_OPT_SCALAR.
 * hgnn_optim_adamw_step: flags = OR of HGNN_OPT_AMSGRAD, HGNN_OPT_CLIP (g' = g state[HGNN_OPT_COEF]; without it
 *   state may be NULL and g' = g), HGNN_OPT_ZERO_GRADS (0 is stored to g after it is read), HGNN_OPT_WRITE_GRADS (g'
 *   is stored to g: the in-place clip; excludes ZERO_GRADS), HGNN_OPT_SCALAR (no 16-byte accesses).  The three state
 *   buffers must be 16-byte aligned; max_exp_avg_sq may be NULL without HGNN_OPT_AMSGRAD.  One launch.
 * Both launch asynchronously, allocate nothing, never synchronise and read nothing back.
 * hgnn_optim_workspace_bytes: device scratch of hgnn_optim_grad_norm (independent of n_chunks).
 * ------------------------------------------------------------------------ */
#define HGNN_OPT_CHUNK 4096
#define HGNN_OPT_AMSGRAD 1
#define HGNN_OPT_CLIP 2
#define HGNN_OPT_ZERO_GRADS 4
#define HGNN_OPT_WRITE_GRADS 8
#define HGNN_OPT_SCALAR 16
#define HGNN_OPT_ST_NONFINITE 1
#define HGNN_OPT_NORM 0
#define HGNN_OPT_COEF 1
#define HGNN_OPT_SUMSQ 2
#define HGNN_OPT_STATE 4
typedef struct hgnn_opt_entry {
    float* p;
    float* g;
    int64_t offset;
    int64_t numel;
    int64_t first_chunk;
    float decay, step_size, inv_sqrt_bc2, one_minus_b1, b2, one_minus_b2, eps;
    int32_t reserved;
} hgnn_opt_entry;
int hgnn_sizeof_opt_entry(void);
int hgnn_optim_workspace_bytes(int64_t n_chunks, size_t* bytes);
int hgnn_optim_grad_norm(const hgnn_opt_entry* host_table, const hgnn_opt_entry* table, int64_t n_tensors,
                         int64_t n_chunks, double max_norm, int32_t flags, double* state, int32_t* status,
                         void* workspace, size_t workspace_bytes, hgnn_stream_t stream);
int hgnn_optim_adamw_step(const hgnn_opt_entry* host_table, const hgnn_opt_entry* table, int64_t n_tensors,
                          int64_t n_chunks, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq,
                          int64_t state_numel, int32_t flags, const double* state, hgnn_stream_t stream);

/* ------------------------------------------------------------------------
 * Graph construction after the neighbour search (reference Modules/gnn_utils.py:193-216, DynamicGraphConstruction):
 * the edge list of a kNN result and the attention weights of its edges.  Added under ABI 26: additions only.
 *
 * hgnn_knn_edges: idx int64 [nq, K] as hgnn_knn_radius_* write it (ids in [0, n_pts), -1 = empty slot; the valid
 *   slots need not be a prefix of their row).  edges int64 [2, cap], cap >= nq K (sym = 0) or 2 nq K (sym = 1): the
 *   first B entries of both rows are written, B = count_and_status[0].
 *     sym = 0: the pairs (row, idx[row, j]) of the valid slots in row-major order.
 *     sym = 1: the union of (s, d) and (d, s) over the valid slots, duplicates removed, ascending in (s, d): the keys
 *       (s << b | d), b = ceil(log2(max(nq, n_pts))), are sorted over their 2 b bits plus one for the empty-slot marker.
 *   count_and_status device int64[2], cleared first: the edge count, and HGNN_GC_ST_BAD_ID when an id is >= n_pts or
 *   < -1 (such a slot is skipped, never used as an address).  max(nq, n_pts) <= 2^31 and nq K < 2^30, else
 *   HGNN_ERR_INVALID_ARG.  Runs on `stream` out of `workspace`: no allocation, no synchronisation, no read-back; the
 *   only atomic is an integer OR into the status word.
 * hgnn_knn_edges_workspace_bytes: device scratch of one call.  Computed on the host from the sizes, but it includes
 *   rocprim's own scratch, whose size rocprim derives from the current device: the call needs the HIP runtime and a
 *   device (as hgnn_graph_intersection_workspace_bytes and hgnn_assign_match_workspace_bytes do); the argument checks
 *   come first.  hgnn_graph_attention_workspace_bytes is a pure host function.
 *
 * hgnn_graph_attention_forward: for E edges (a_e, b_e) = (graph[e], graph[E + e]) (int32 or int64 by index_dtype),
 *   A float32 [Na, D], B float32 [Nb, D] (may be the same pointer), 1 <= D <= HGNN_GA_MAX_DIM:
 *     x_e = <A[a_e], B[b_e]>                         bit-equal to hgnn_edge_dot_f32; 0 for an id out of range
 *     z_e = bn_weight[0] (x_e - mu) rstd + bn_bias[0],  rstd = 1 / sqrt(var + eps)
 *     f_e = sigmoid(z_e) (HGNN_GA_FN_SIGMOID) | exp(z_e) (HGNN_GA_FN_EXP)
 *     w_e = f_e / (sum f / E) with HGNN_GA_NORM, else f_e
 *   With HGNN_GA_TRAINING (E >= 2) mu and the biased var are the batch's, from float64 sums of x and x^2, and the
 *   call then updates the running statistics as nn.BatchNorm1d does: num_batches_tracked += 1 (may be NULL),
 *   running = (1 - m) running + m (mu | var E / (E - 1)), m = momentum, or 1 / num_batches_tracked for momentum < 0.
 *   Without it mu and var are running_mean[0] and running_var[0] and nothing but the outputs is written.  Every sum
 *   is float64 in a fixed order that depends on E alone: two calls give the same bits.  Outputs: x, logits (z),
 *   weights float32 [E]; state device double[HGNN_GA_STATE] (indices below).  All BatchNorm arguments are device
 *   pointers.  E = 0 without HGNN_GA_TRAINING does nothing.
 * hgnn_graph_attention_backward: g_w float32 [E], g_logits float32 [E] or NULL; state as the forward wrote it (the
 *   entries HGNN_GA_DBETA, HGNN_GA_DGAMMA, HGNN_GA_SGF are written here).  With m = sum f / E, xhat = (x - mu) rstd:
 *     g_f = g_w / m - (sum g_w f) / (E m^2)   (g_w without HGNN_GA_NORM);   G = g_f phi'(z) + g_logits
 *     g_bn = (dgamma, dbeta) = (sum G xhat, sum G)
 *     g_x = gamma rstd (G - dbeta / E - xhat dgamma / E) with HGNN_GA_TRAINING, gamma rstd G without
 *   g_x float32 [E] is d loss / d x; dA and dB follow from it by hgnn_segment_reduce_f32 over the plans of the two
 *   graph rows, as for hgnn_edge_dot_f32.  No atomics.
 * Both launch asynchronously, allocate nothing, never synchronise and read nothing back.
 * hgnn_graph_attention_workspace_bytes: device scratch of one forward (backward = 0) or backward (1) call.
 * ------------------------------------------------------------------------ */
#define HGNN_GC_ST_BAD_ID 1
#define HGNN_GA_MAX_DIM 16
#define HGNN_GA_FN_SIGMOID 0
#define HGNN_GA_FN_EXP 1
#define HGNN_GA_TRAINING 1
#define HGNN_GA_NORM 2
#define HGNN_GA_MEAN 0
#define HGNN_GA_VAR 1      /* biased */
#define HGNN_GA_RSTD 2
#define HGNN_GA_SUMF 3
#define HGNN_GA_E 4
#define HGNN_GA_DBETA 5
#define HGNN_GA_DGAMMA 6
#define HGNN_GA_SGF 7      /* sum g_w f */
#define HGNN_GA_STATE 8
int hgnn_knn_edges_workspace_bytes(int64_t nq, int32_t K, int64_t n_pts, int32_t sym, size_t* bytes);
int hgnn_knn_edges(const int64_t* idx, int64_t nq, int32_t K, int64_t n_pts, int32_t sym, int64_t* edges, int64_t cap,
                   int64_t* count_and_status, void* workspace, size_t workspace_bytes, hgnn_stream_t stream);
int hgnn_graph_attention_workspace_bytes(int64_t E, int32_t backward, size_t* bytes);
int hgnn_graph_attention_forward(const float* A, int64_t Na, const float* B, int64_t Nb, int32_t D, const void* graph,
                                 int32_t index_dtype, int64_t E, const float* bn_weight, const float* bn_bias,
                                 float* running_mean, float* running_var, int64_t* num_batches_tracked, double eps,
                                 double momentum, int32_t flags, int32_t fn, float* x, float* logits, float* weights,
                                 double* state, void* workspace, size_t workspace_bytes, hgnn_stream_t stream);
int hgnn_graph_attention_backward(const float* x, int64_t E, const float* bn_weight, const float* bn_bias,
                                  int32_t flags, int32_t fn, double* state, const float* g_w, const float* g_logits,
                                  float* g_x, float* g_bn, void* workspace, size_t workspace_bytes,
                                  hgnn_stream_t stream);

/* ------------------------------------------------------------------------
 * Event preparation (reference Modules/utils.py:57-108, TrackMLDataset.__getitem__) on the device: the noise / pT /
 * isolated-hit masks, nhits per particle, signal_mask, and the compaction and re-indexing of edge lists and node
 * fields.  Added under ABI 26: additions only.  Every entry launches on `stream`, allocates nothing, never
 * synchronises and reads nothing back; rocprim's scratch comes out of the caller's workspace (the size queries need the
 * HIP runtime and a device, as hgnn_knn_edges_workspace_bytes does; their argument checks come first).  No float
 * atomics: every output is a deterministic function of the inputs.  N < 2^31 and E < 2^31, else
 * HGNN_ERR_INVALID_ARG; N = 0 or E = 0 is HGNN_OK with zero counts.  bool / flag arrays are one byte per element.
 *
 * hgnn_event_hit_counts: nhits[i] = the number of j with pid[j] == pid[i] (pid int64 [N], any values; 0 is a particle
 *   like any other).  A stable radix sort of (pid, position) over all 64 key bits, run heads, run lengths, scattered
 *   back.  With signal_mask != NULL also signal_mask[i] = nhits[i] >= n_hits && (primary == NULL || primary[i] == 1).
 * hgnn_event_nodes: the node stage.  keep[i] =
 *       (HGNN_EP_NOISE ? true : pid[i] != 0)
 *    && (hard_ptcut > 0 ? pt[i] > (float)hard_ptcut : true)      the ORIGINAL pt, compared in float32; NaN fails
 *    && (HGNN_EP_REMOVE_ISOLATED ? i occurs in edge_index [2, E] : true)
 *   new_id int32 [N]: the exclusive scan of keep, -1 where not kept.  pt_out[i] = pid[i] == 0 ? 0 : pt[i].
 *   nhits int64 [N] and signal_mask [N] as hgnn_event_hit_counts writes them (primary is read iff
 *   HGNN_EP_USE_PRIMARY), both full length.  info device int64[HGNN_EP_INFO] is cleared first; then
 *   info[HGNN_EP_N_NODES] = the number of kept hits, and info[HGNN_EP_STATUS] |= HGNN_EP_ST_BAD_ID when an id of
 *   edge_index is outside [0, N) (read only with HGNN_EP_REMOVE_ISOLATED; such an id marks nothing and is never used
 *   as an address).  edge_index may be NULL without HGNN_EP_REMOVE_ISOLATED.
 * hgnn_event_inverse_mask: inverse_mask int64 [cap] = the kept positions ascending (inverse_mask[new_id[i]] = i for
 *   every new_id[i] in [0, cap)).
 * hgnn_event_edges_count: the edge stage of one list edges int64 [2, E].  Edge e = (a, b) is kept iff both ids are in
 *   [0, N), new_id[a] >= 0, new_id[b] >= 0 and (edge_keep == NULL || edge_keep[e] != 0).  Writes *count (device
 *   int64) = the number of kept edges and ORs HGNN_EP_ST_BAD_ID into *status (device int64, NOT cleared) when an id
 *   of ANY edge of the list, kept or not, is outside [0, N); that edge is dropped and the id never used as an address.
 *   The kept edges' positions (an exclusive scan: output order = input order) stay in the workspace for
 *   hgnn_event_edges_fill, which must be given the same workspace, untouched, and the same edges / E / edge_keep /
 *   new_id / N.  Another list can be filtered against the same new_id without redoing the node stage.
 * hgnn_event_edges_fill: out int64 [2, cap] receives (new_id[a], new_id[b]) of every kept edge whose position is
 *   < cap, and y_out[p] = y[e], y_pid_out[p] = y_pid[e] where those pointers are not NULL.
 * hgnn_event_gather_rows: out[r, :] = src[index[r], :] for rows of `cols` elements of elem_bytes = 1, 4 or 8; a row
 *   whose index is outside [0, n_rows) is zero-filled.  Needs no workspace.
 * ------------------------------------------------------------------------ */
#define HGNN_EP_ST_BAD_ID 1
#define HGNN_EP_NOISE 1
#define HGNN_EP_REMOVE_ISOLATED 2
#define HGNN_EP_USE_PRIMARY 4
#define HGNN_EP_N_NODES 0
#define HGNN_EP_E_EDGE_INDEX 1
#define HGNN_EP_E_MODULEWISE 2
#define HGNN_EP_E_SIGNAL 3
#define HGNN_EP_STATUS 4
#define HGNN_EP_INFO 8
int hgnn_event_hit_counts_workspace_bytes(int64_t N, size_t* bytes);
int hgnn_event_hit_counts(const int64_t* pid, const int64_t* primary, int64_t N, int64_t n_hits, int64_t* nhits,
                          uint8_t* signal_mask, void* workspace, size_t workspace_bytes, hgnn_stream_t stream);
int hgnn_event_nodes_workspace_bytes(int64_t N, int64_t E, size_t* bytes);
int hgnn_event_nodes(const int64_t* pid, const float* pt, const int64_t* primary, const int64_t* edge_index,
                     int64_t N, int64_t E, double hard_ptcut, int64_t n_hits, int32_t flags, int32_t* new_id,
                     float* pt_out, int64_t* nhits, uint8_t* signal_mask, int64_t* info, void* workspace,
                     size_t workspace_bytes, hgnn_stream_t stream);
int hgnn_event_inverse_mask(const int32_t* new_id, int64_t N, int64_t* inverse_mask, int64_t cap,
                            hgnn_stream_t stream);
int hgnn_event_edges_workspace_bytes(int64_t E, size_t* bytes);
int hgnn_event_edges_count(const int64_t* edges, int64_t E, const uint8_t* edge_keep, const int32_t* new_id,
                           int64_t N, int64_t* count, int64_t* status, void* workspace, size_t workspace_bytes,
                           hgnn_stream_t stream);
int hgnn_event_edges_fill(const int64_t* edges, int64_t E, const uint8_t* edge_keep, const int32_t* new_id, int64_t N,
                          const uint8_t* y, const uint8_t* y_pid, int64_t* out, int64_t cap, uint8_t* y_out,
                          uint8_t* y_pid_out, const void* workspace, size_t workspace_bytes, hgnn_stream_t stream);
int hgnn_event_gather_rows(const void* src, int64_t n_rows, int32_t cols, int32_t elem_bytes, const int64_t* index,
                           int64_t n_out, void* out, hgnn_stream_t stream);

/* ------------------------------------------------------------------------
 * Training pairs of the embedding stage (reference GNNEmbedding/embedding_base.py:109-135, get_training_samples)
 * from the kNN matrix, row by row: no [2, N*K] prediction graph and no sort of the pairs (csrc/trainpairs.hip).
 * Added under ABI 26: additions only.  Every entry launches on `stream`, allocates nothing, never synchronises and
 * reads nothing back (the size query needs the HIP runtime and a device for rocprim's scratch sizes; its argument
 * checks come first).  No atomic decides a position: the output is a deterministic function of the inputs.
 *
 * idx int64 [n, K], 1 <= K <= HGNN_TP_MAX_K: ids in [0, n), -1 = empty slot (anywhere in a row), duplicates allowed.
 * mte int64 [2, t]; signal_mask one byte per hit [n]; pid int64 [n].  n < 2^31, t < 2^29 and n K + 2 t < 2^31, else
 * HGNN_ERR_INVALID_ARG.  e_bidir = the columns of [mte, mte.flip(0)] whose two ends pass signal_mask, in that order.
 *   HGNN_TP_MODE_MODULEWISE: for row i ascending, its DISTINCT valid ids j ascending with (i, j) not in e_bidir and
 *     (pid[i] != pid[j] || pid[i] == 0 || pid[j] == 0), y = 0; then all of e_bidir, y = 1.
 *   HGNN_TP_MODE_PID: for row i ascending, every valid slot j in slot order with !(signal_mask[i] && signal_mask[j])
 *     and !(pid[i] == pid[j] && pid[i] != 0 && pid[j] != 0), y = 0; nothing of e_bidir (its pairs pass the mask).
 * hgnn_training_pairs_count: info device int64[HGNN_TP_INFO] = {P, the pairs of the row part, the pairs of the
 *   e_bidir part, status}.  status: HGNN_TP_ST_BAD_IDX when an entry of idx is outside [-1, n), HGNN_TP_ST_BAD_MTE
 *   when an id of mte is outside [0, n) (checked in both modes); such a slot or column is skipped and the id never
 *   used as an address.  The sorted e_bidir keys and the scanned positions stay in the workspace for
 * hgnn_training_pairs_fill, which must be given the same workspace, untouched, and the same inputs: out_graph int64
 *   [2, cap] and out_y uint8 [cap] receive every pair whose position is < cap (cap = P: exactly the result).
 * ------------------------------------------------------------------------ */
#define HGNN_TP_MAX_K 128
#define HGNN_TP_MODE_MODULEWISE 0
#define HGNN_TP_MODE_PID 1
#define HGNN_TP_ST_BAD_IDX 1
#define HGNN_TP_ST_BAD_MTE 2
#define HGNN_TP_P 0
#define HGNN_TP_N_ROW 1
#define HGNN_TP_N_TRUTH 2
#define HGNN_TP_STATUS 3
#define HGNN_TP_INFO 4
int hgnn_training_pairs_workspace_bytes(int64_t n, int32_t K, int64_t t, int32_t mode, size_t* bytes);
int hgnn_training_pairs_count(const int64_t* idx, int64_t n, int32_t K, const int64_t* mte, int64_t t,
                              const uint8_t* signal_mask, const int64_t* pid, int32_t mode, int64_t* info,
                              void* workspace, size_t workspace_bytes, hgnn_stream_t stream);
int hgnn_training_pairs_fill(const int64_t* idx, int64_t n, int32_t K, const int64_t* mte, int64_t t,
                             const uint8_t* signal_mask, const int64_t* pid, int32_t mode, int64_t* out_graph,
                             uint8_t* out_y, int64_t cap, const void* workspace, size_t workspace_bytes,
                             hgnn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HGNN_HIP_H */
