/*
 * gsparse.h -- C ABI of libgsparse.so, the MI355X (gfx950) edge-scoring engine.
 *
 * This is the drop-in boundary below the reference's Python API
 * (/root/reference/src/sparsification): the host mirror
 * gnn-sparsification-research_amd/gsparse/ binds these entry points with
 * ctypes and keeps the reference's names, argument meaning and error
 * behaviour.  The reference has no FFI of its own (it is NumPy/SciPy), so
 * each entry point below cites the reference function whose arithmetic it
 * replaces.  Conventions:
 *   - every function returns 0 (GS_OK) or a negative GS_E* code and never
 *     throws; gs_last_error() gives the message (thread-local);
 *   - "loc" arguments say where a pointer lives: GS_HOST or GS_DEVICE;
 *   - scores are float64, one per canonical-CSR entry, in CSR order
 *     (the reference's adj.nonzero() order, metrics.py:47,115,236,348);
 *   - calls are synchronous with respect to host pointers; device-pointer
 *     outputs are complete when the call returns unless gs_set_async(1).
 */
#ifndef GSPARSE_H
#define GSPARSE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS_API_VERSION 3

enum {
    GS_OK = 0,
    GS_EINVAL = -1,       /* bad argument (Python shim raises ValueError)      */
    GS_EHIP = -2,         /* HIP runtime error                                 */
    GS_ENOMEM = -3,       /* device allocation failed                          */
    GS_ESTATE = -4,       /* call out of order (e.g. no graph set)             */
    GS_EUNSUPPORTED = -5, /* input outside the implemented contract            */
    GS_EINDEX = -6,       /* an array shorter than the index range it must cover
                             (Python shim raises IndexError, as NumPy does)     */
    GS_ENOCONV = -7       /* an iterative solver stopped at its cap unconverged;
                             no value is returned (Python shim: RuntimeError)   */
};

enum { GS_HOST = 0, GS_DEVICE = 1 };

typedef struct gs_ctx gs_ctx;

/* ---- library / context ------------------------------------------------- */
int gs_api_version(void);
const char *gs_last_error(void);
int gs_device_count(int *count);
/* One context per (process, device); not re-entrant per context. */
int gs_create(int device, gs_ctx **out);
void gs_destroy(gs_ctx *ctx);
/* Use an external hipStream_t (e.g. torch.cuda.current_stream()); NULL =
 * the context's own stream. */
int gs_set_stream(gs_ctx *ctx, void *hip_stream);
/* Stream ordering without a host sync (hip_stream NULL = the null stream):
 * gs_stream_wait -- work the context enqueues from now on runs after
 *   everything already enqueued on hip_stream (call it before handing the
 *   library device buffers that another stream produced or last used, e.g.
 *   torch.cuda.current_stream());
 * gs_stream_signal -- work enqueued on hip_stream from now on runs after
 *   everything the context has enqueued (device outputs in async mode). */
int gs_stream_wait(gs_ctx *ctx, void *hip_stream);
int gs_stream_signal(gs_ctx *ctx, void *hip_stream);
int gs_synchronize(gs_ctx *ctx);
/* 1: device-pointer outputs may still be in flight on return. */
int gs_set_async(gs_ctx *ctx, int async_);

/* Kernel timing on the context's stream (hipEvents around every launch). */
int gs_profile_enable(gs_ctx *ctx, int on);
int gs_profile_reset(gs_ctx *ctx);
/* i-th profiled kernel name; -1 past the end. ms = summed launch time. */
int gs_profile_get(gs_ctx *ctx, int i, char *name, int name_len, int64_t *launches,
                   double *ms, double *bytes);

/* ---- graph --------------------------------------------------------------
 * Replaces GraphSparsifier.__init__'s COO->CSR build (core.py:70-74):
 * sp.csr_matrix((ones(E), (ei[0], ei[1])), (n, n)) -- duplicates summed
 * (data = multiplicity), columns sorted.  Built on the device.
 * GS_EINVAL: negative n or E, an id outside [0, n); GS_EUNSUPPORTED: n >= 2^31.
 *
 * A refused graph call (either entry point, any error code) leaves the EMPTY
 * graph resident -- gs_graph_shape reports n = nnz = 0 -- under a new graph
 * epoch: neither the graph set before it, nor anything cached or derived from
 * it, nor any part of the refused arrays is used by a later call. */
int gs_graph_from_edge_index(gs_ctx *ctx, int64_t n, int64_t E, const int64_t *src,
                             const int64_t *dst, int loc);
/* Canonical CSR given directly (sorted columns, no duplicates), e.g. the
 * adj argument of the metrics.py module functions. data may be NULL (=1).
 * Validated on the device before it becomes the resident graph.  GS_EINVAL:
 * indptr[0] != 0, indptr[n] != nnz, a row whose ends are not in order inside
 * [0, nnz] (no index entry of such a row is read), a column outside [0, n);
 * GS_EUNSUPPORTED: a row with unsorted or duplicate columns, n >= 2^31. */
int gs_graph_from_csr(gs_ctx *ctx, int64_t n, int64_t nnz, const int64_t *indptr,
                      const int32_t *indices, const double *data, int loc);
int gs_graph_shape(gs_ctx *ctx, int64_t *n, int64_t *nnz, int *symmetric);
/* Canonical edge list for the dataset loader (gsparse/loader.py, standing in
 * for the reference's absent src/data; PyG's to_undirected + coalesce):
 * undirected != 0 adds every reversed pair; remove_self_loops != 0 drops
 * u == v; the result is sorted by (row, col) with duplicates removed.
 * *out_E: capacity on entry (2E suffices), edge count on return. */
int gs_coalesce_edges(gs_ctx *ctx, int64_t n, int64_t E, const int64_t *src, const int64_t *dst,
                      int undirected, int remove_self_loops, int64_t *out_src, int64_t *out_dst,
                      int64_t *out_E, int loc);
int gs_graph_copy_csr(gs_ctx *ctx, int64_t *indptr, int32_t *indices, double *data, int loc);

/* ---- scorers: out[e - e0] for CSR entries e in [e0, e1) ------------------ */
/* calculate_jaccard_scores, metrics.py:17-64 (bit-exact). */
int gs_jaccard(gs_ctx *ctx, int64_t e0, int64_t e1, double *out, int loc);
/* Part `part` of `nparts` of the whole-graph Jaccard (multi-GPU sharding,
 * SURVEY 8(e)): out[nnz] holds this part's pairs (both CSR entries of each
 * undirected pair on a symmetric graph; an edge range on a directed one) and
 * 0.0 elsewhere, so the element-wise sum of the nparts outputs equals
 * gs_jaccard(0, nnz) bit for bit. */
int gs_jaccard_part(gs_ctx *ctx, int part, int nparts, double *out, int loc);
/* Sharded Jaccard with an all-gather of per-pair counts (multi-GPU, SURVEY
 * 8(e); symmetric graphs, else GS_EUNSUPPORTED).  The owner of an undirected
 * pair {u, v} is the endpoint of larger degree (ties: smaller id); its CSR
 * entry (u, v) is the pair's owner entry.  Part p of nparts owns the owner
 * entries of rows [row_cut[p], row_cut[p+1]) -- contiguous row ranges cut at
 * equal shares of the intersection work, the same on every rank -- which are
 * owner entries [owner_off[p], owner_off[p+1]) in CSR order.
 *   gs_jaccard_shares: row_cut[nparts+1], owner_off[nparts+1] (host; either
 *     may be NULL).
 *   gs_jaccard_part_counts: counts[i] = |N(u) ∩ N(v)| of part p's i-th owner
 *     entry (uint32, owner_off[p+1] - owner_off[p] values).
 *   gs_jaccard_from_counts: every part's counts (part p's at counts + p*stride,
 *     e.g. an all-gather of the shares padded to stride) -> out[nnz], the
 *     score of both CSR entries of every pair (the reference's single fp64
 *     division of metrics.py:54-59): bit-identical to gs_jaccard(0, nnz).
 *     A part longer than stride is GS_EINDEX. */
int gs_jaccard_shares(gs_ctx *ctx, int nparts, int64_t *row_cut, int64_t *owner_off);
int gs_jaccard_part_counts(gs_ctx *ctx, int part, int nparts, uint32_t *counts, int loc);
int gs_jaccard_from_counts(gs_ctx *ctx, int nparts, const uint32_t *counts, int64_t stride,
                           int c_loc, double *out, int loc);
/* Distributed global top-k of Jaccard-T (GraphSparsifier.sparsify, core.py:229-240, over N
 * ranks; SURVEY 8(e) "top-k alone: histogram all-reduce") without gathering scores.  Each
 * rank selects over its own owner pairs (gs_jaccard_part_counts; a pair's two CSR entries
 * share one score, multiplicity 2, a self-loop 1):
 *   gs_jsel_begin   scores (scores may be NULL: this part's pairs, owner order) and keys of
 *                   the own pairs; hist (device, GS_JSEL_BINS uint64) = the weighted
 *                   histogram of the keys' top 12 bits.  0 < num_keep < nnz.
 *   gs_jsel_step    hist holds the SUM over ranks of the last histogram: picks the digit
 *                   of the cut's rank and writes the next digit's histogram into hist;
 *                   GS_JSEL_PASSES calls (12 + 4 x 13 bits), *passes_left counts down.
 *   gs_jsel_result  the cut score, the entries strictly beyond it and the tie block (the
 *                   same on every rank, = gs_topk_mask's), and this rank's tied positions.
 *   gs_jsel_tie_positions  this rank's tied CSR positions (npos >= my_tied).
 *   gs_jsel_keep    2-bit keep codes of the own pairs (bit 0 the owner entry, bit 1 the
 *                   reverse entry), pair i in bits 2 (i % 4) of byte i / 4: ceil(pairs / 4)
 *                   bytes.  need = num_keep - n_beyond; when 0 < need < n_tied the cut is
 *                   ambiguous and tie_pos must hold every rank's tied positions (ntie =
 *                   n_tied, any order): the block is resolved as np.argsort(kind='stable')
 *                   resolves it (top: the highest positions; keep_lowest: the lowest).
 *   gs_jsel_mask    every rank's codes (part p's at keep_all + p * stride bytes, an
 *                   all-gather padded to stride) -> the CSR keep mask mask[nnz], bit-identical
 *                   to gs_topk_mask on the gathered scores.
 * Symmetric graphs with nnz < 2^31 (else GS_EUNSUPPORTED). */
enum { GS_JSEL_BINS = 8192, GS_JSEL_PASSES = 5 };
int gs_jsel_begin(gs_ctx *ctx, int part, int nparts, const uint32_t *counts, int c_loc,
                  int64_t num_keep, int keep_lowest, uint64_t *hist, double *scores, int s_loc);
int gs_jsel_step(gs_ctx *ctx, uint64_t *hist, int *passes_left);
int gs_jsel_result(gs_ctx *ctx, double *cut, int64_t *n_beyond, int64_t *n_tied, int64_t *my_tied);
int gs_jsel_tie_positions(gs_ctx *ctx, int64_t *pos, int64_t npos, int loc);
int gs_jsel_keep(gs_ctx *ctx, const int64_t *tie_pos, int64_t ntie, int t_loc, int64_t need,
                 uint8_t *keep, int k_loc);
int gs_jsel_mask(gs_ctx *ctx, int nparts, const uint8_t *keep_all, int64_t stride, int k_loc,
                 uint8_t *mask, int m_loc);
/* calculate_adamic_adar_scores, metrics.py:67-121 (bit-exact).  c[w] =
 * 1/sqrt(max(log(deg_w+1),1e-10)) as NumPy computes it (metrics.py:104-108),
 * n values. */
int gs_adamic_adar(gs_ctx *ctx, const double *c, int c_loc, int64_t e0, int64_t e1,
                   double *out, int loc);
/* compute_scores('degree'), core.py:167-172 (bit-exact). */
int gs_degree(gs_ctx *ctx, int64_t e0, int64_t e1, double *out, int loc);
/* calculate_feature_cosine_scores, metrics.py:301-358 (bit-exact, x's dtype). */
int gs_feature_cosine_f32(gs_ctx *ctx, const float *x, int64_t f, int x_loc, int64_t e0,
                          int64_t e1, double *out, int loc);
int gs_feature_cosine_f64(gs_ctx *ctx, const double *x, int64_t f, int x_loc, int64_t e0,
                          int64_t e1, double *out, int loc);

/* ---- ApproxER: calculate_approx_effective_resistance_scores,
 *      metrics.py:178-298 -------------------------------------------------
 * gs_er_prepare: edges u<v in CSR order (m of them, :236-242), L_reg =
 *   diag(rowsum A) - A + reg*I (:251-256); allocates Y/Z (n x k, row-major).
 * gs_er_project_rows: streams rows [e0, e1) of the raw standard-normal
 *   matrix (row-major, k per row, NumPy Generator order) and folds
 *   Y = B @ (raw / sqrt_k) (:272-275) in ascending edge id.  Rows must be
 *   streamed in order, each exactly once.
 * gs_er_project_pcg64: the same, drawing the normals on the device from
 *   NumPy's PCG64 state (state_hi/lo, inc_hi/lo) with NumPy's ziggurat.
 * gs_er_solve: CG on columns [col0, col1) (:284-289), SciPy 1.15 cg
 *   recurrence with OpenBLAS-SkylakeX ddot order for blas_threads threads
 *   (more than 64 run as 64: OpenBLAS's MAX_THREADS in NumPy's build).
 * gs_er_scores: out[e-e0] = sum over columns [col0,col1) of (Z_u - Z_v)^2 in
 *   NumPy pairwise order (:292-293).  [col0,col1) must be a node of the
 *   pairwise tree of k (the whole range, or a gs_er_split() block); when
 *   finalize != 0 the clamp of :296-297 is applied.
 * gs_er_iterations: CG iterations each column ran (k values).
 * gs_er_copy_z: the solved Z columns [col0, col1) (metrics.py:285-289's
 *   Z[:, i] = cg(...)), n rows x (col1 - col0) row-major -- a parity read-out. */
int gs_er_prepare(gs_ctx *ctx, int64_t k, double reg, int64_t *m_out);
int gs_er_project_rows(gs_ctx *ctx, int64_t e0, int64_t e1, const double *raw, int loc,
                       double sqrt_k);
int gs_er_project_pcg64(gs_ctx *ctx, uint64_t state_hi, uint64_t state_lo, uint64_t inc_hi,
                        uint64_t inc_lo, double sqrt_k);
/* Column-slice forms (a rank's JL columns): the normal stream /
 * the host rows are the same whole NumPy stream, but only Y[:, col0:col1] is
 * formed; gs_er_solve then accepts column ranges inside [col0, col1). */
int gs_er_project_pcg64_cols(gs_ctx *ctx, uint64_t state_hi, uint64_t state_lo, uint64_t inc_hi,
                             uint64_t inc_lo, double sqrt_k, int64_t col0, int64_t col1);
int gs_er_project_rows_cols(gs_ctx *ctx, int64_t e0, int64_t e1, const double *raw, int loc,
                            double sqrt_k, int64_t col0, int64_t col1);
int gs_er_solve(gs_ctx *ctx, int64_t col0, int64_t col1, int32_t maxiter, double rtol,
                int32_t blas_threads);
int gs_er_scores(gs_ctx *ctx, int64_t col0, int64_t col1, int64_t e0, int64_t e1,
                 int finalize, double *out, int loc);
int gs_er_iterations(gs_ctx *ctx, int32_t *iters, int loc);
int gs_er_copy_z(gs_ctx *ctx, int64_t col0, int64_t col1, double *out, int loc);
/* Column blocks of the pairwise tree of k at depth log2(parts): bounds has
 * parts+1 entries.  parts must be a power of two. */
int gs_er_split(int64_t k, int32_t parts, int64_t *bounds);
/* The plan gs_er_solve follows for ncols columns of an n-row system whose L_reg has
 * lnnz entries, with blas_threads ddot threads and the GSPARSE_CG_* / GSPARSE_RES_* /
 * GSPARSE_REG_* variables as they are now: out = {solver mode 0..5, columns per lane,
 * chain rows per trip, BLAS chunks}.  Host code only: needs no context and no device. */
int gs_er_plan(int64_t n, int64_t lnnz, int64_t ncols, int32_t blas_threads, int32_t out[4]);
/* Where the register-resident solver (mode 5) keeps p for an n-row system with
 * blas_threads ddot threads, under GSPARSE_REG_NT / GSPARSE_REG_KEEP as they are now;
 * unit: the unit-weight form whose diagonals follow from the entry counts.  out[0..7] =
 * {threads per workgroup (0: mode 5 does not apply; the rest is then 0), threads per
 * chain G, row slots per thread, BLAS chunks T, LDS slots of p (the zero slot's index),
 * diagonal slots, LDS bytes of a launch, 0}; then four blocks of 16 per-chunk values:
 * first row, rows, leading rows whose p is in LDS, LDS slot of the first row.  Host code
 * only: needs no context and no device. */
int gs_er_reg_layout(int64_t n, int32_t blas_threads, int32_t unit, int64_t out[72]);

/* As gs_er_reg_layout with a p window of `window` wave-slots per chunk asked for (3 or 4):
 * out[7] = the window laid out -- 0 where the window kernel does not exist (other than
 * two threads per chain; the weighted form) or a prefix is not a whole number of
 * wave-slots, and the layout is then gs_er_reg_layout's -- and a fifth block of 16: the
 * LDS slot each chunk's window starts at. */
int gs_er_reg_layout_w(int64_t n, int32_t blas_threads, int32_t unit, int32_t window, int64_t out[88]);

/* What the last register-resident solve chose for its p window (GSPARSE_REG_WINDOW):
 * out = {window in wave-slots (0: the plain layout), wave-slots with a global p code
 * under the plain layout, under the windowed one (-1 each where no window was weighed),
 * window codes in the ELL copy}. */
int gs_er_reg_window(gs_ctx *c, int64_t out[4]);

/* ---- selection: GraphSparsifier.sparsify core.py:229-242 -----------------
 * mask[E] (uint8): the num_keep highest (keep_lowest: lowest) of the nnz
 * scores, ties broken as np.argsort(kind='stable') does (top: highest
 * indices; lowest: lowest indices); num_keep == 0 keeps all nnz for top
 * (the reference's idx[-0:] quirk) and none for keep_lowest.  Also returns
 * the cut key, #strictly-beyond-cut and #tied-at-cut (n_tied > needed means
 * the reference's unstable argsort may resolve the tie block differently). */
int gs_topk_mask(gs_ctx *ctx, const double *scores, int s_loc, int64_t nnz, int64_t E,
                 int64_t num_keep, int keep_lowest, uint8_t *mask, int m_loc,
                 double *cut, int64_t *n_beyond, int64_t *n_tied);

/* ---- metric backbone: compute_metric_backbone, metric_backbone.py:28-141
 * keep[idx] for every edge_index column idx=(src,dst): shortest-path
 * distance d from src in the undirected graph of the src<dst columns
 * (min weight over duplicates), keep iff d == inf or w[idx] <= d + eps.
 * nw = number of entries of w: nw < E is GS_EINDEX (the reference reads
 * edge_weights[idx] for every column, metric_backbone.py:73-74, and raises
 * IndexError).  n_relax (optional) returns the number of edge relaxations
 * performed. */
/* sparsify_degree_aware phase 1 (core.py:415-428) for min_edges_per_node = 1
 * (any other budget: gs_segment_topk below): for every node u, pick[u] = the edge_index column i (src[i] == u) holding
 * the unique maximum of scores[i], -1 if u has no column, -2 when the
 * reference's np.argsort order decides (ties at the maximum or a NaN).
 * scores are indexed by column as the reference indexes them (needs E <=
 * nscores, else GS_EINVAL, the reference's IndexError). */
int gs_segment_argmax(gs_ctx *ctx, const double *scores, int s_loc, int64_t nscores,
                      const int64_t *src, int src_loc, int64_t E, int64_t n, int64_t *pick,
                      int pick_loc);

/* sparsify_degree_aware phase 1 for any min_edges_per_node = k >= 1
 * (core.py:415-428): a segmented top-k.  For every node u with d columns
 * (src[i] == u), the set of its min(k, d) highest-scoring columns, on the
 * keys of gs_topk_mask (-0.0 == +0.0, NaN the largest key):
 *   d <= k: all its columns, status 1 (never ambiguous);
 *   d >  k: t = the k-th largest key, gt = keys above t, eq = keys equal to t;
 *           gt + eq == k: the columns with key >= t, status 1; otherwise, or
 *           with a NaN in the segment, the reference's np.argsort order decides
 *           inside the tie block: status 2 and none of u's mask bytes is set
 *           (the caller makes the reference's own call for u);
 *   d == 0: status 0.
 * mask[E]: 1 = guaranteed column of a decided node.  n_guaranteed = mask bytes
 * set, n_ambiguous = nodes of status 2.  class_counts[0..ncounts): nodes handled
 * per GS_SEGK_* class (by segment length: SHORT one key per lane of a sub-wave
 * group, LDS one workgroup with the keys staged in LDS, STREAM one workgroup
 * re-reading its keys per radix digit; GSPARSE_SEGK_SHORT_MAX / _LDS_MAX lower
 * the class limits).  A src sorted ascending needs no grouping pass.  Errors as
 * gs_segment_argmax (E > nscores, src out of [0, n): GS_EINVAL); k < 1 is
 * GS_EINVAL. */
enum { GS_SEGK_EMPTY = 0, GS_SEGK_ALL, GS_SEGK_SHORT, GS_SEGK_LDS, GS_SEGK_STREAM, GS_SEGK_CLASSES };
int gs_segment_topk(gs_ctx *ctx, const double *scores, int s_loc, int64_t nscores,
                    const int64_t *src, int src_loc, int64_t E, int64_t n, int64_t k,
                    uint8_t *mask, int mask_loc, uint8_t *status, int status_loc,
                    int64_t *n_guaranteed, int64_t *n_ambiguous, int64_t *class_counts,
                    int ncounts);

/* ---- sampling: GraphSparsifier.sparsify_sampled core.py:333-350 ------------
 * mask[E] (uint8): the set rng.choice(E, size=num_keep, replace=False, p=probs)
 * draws, bit for bit, with probs = maximum(nan_to_num(scores, 1e-8 for NaN and
 * +-inf), 1e-8) / np.sum (the pairwise sums of NumPy's 8192-element buffer blocks,
 * folded in order) and rng a Generator(PCG64) in the
 * state (state_hi/lo, inc_hi/lo): NumPy 2.x's rejection rounds run on the device.
 * Each round rebuilds cdf = cumsum(p) / cumsum(p)[-1] (sequential adds, IEEE
 * divides) with the found entries of p zeroed, draws size - n_uniq doubles
 * ((next_uint64 >> 11) * 2^-53), searches them (side='right') and claims the
 * indices.  *rounds = rounds run, *draws = uint64s of the stream consumed (the
 * generator's state afterwards is the given one advanced by *draws).
 * *status: 0 = the mask was written by the device rounds; 1 = degenerate input,
 * the mask is untouched: a total that is not finite and positive, a p that
 * underflowed to 0, nscores != E, E < 1 or num_keep outside [0, E] -- NumPy
 * raises or takes another branch on each, so the caller makes the reference's
 * own call.  num_keep == 0: an all-zero mask, status 0, 0 rounds, 0 draws.
 * Read-outs of the pieces (parity tests, the same kernels):
 *   gs_pcg64_doubles   out[j] = Generator.random()'s double number offset + j of
 *                      the stream, j < n.
 *   gs_sample_probs    p_out[n] = the normalised probs above, *total_out = the sum
 *                      they were divided by (n >= 1).
 *   gs_cumsum_ordered  out[n] = np.cumsum(p) (not divided; out must not be p).
 * GS_SAMPLE_TILE: elements per LDS tile of the ordered cumsum; GS_SAMPLE_SUBTREE:
 * each block's pairwise tree is cut into subtrees of at most this many terms, one
 * thread each (sizes around both are where the kernels change path). */
enum { GS_SAMPLE_TILE = 1024, GS_SAMPLE_SUBTREE = 2048 };
int gs_sample_mask(gs_ctx *ctx, const double *scores, int s_loc, int64_t nscores, int64_t E,
                   int64_t num_keep, uint64_t state_hi, uint64_t state_lo, uint64_t inc_hi,
                   uint64_t inc_lo, uint8_t *mask, int m_loc, int32_t *status, int64_t *rounds,
                   int64_t *draws);
int gs_pcg64_doubles(gs_ctx *ctx, uint64_t state_hi, uint64_t state_lo, uint64_t inc_hi,
                     uint64_t inc_lo, uint64_t offset, int64_t n, double *out, int loc);
int gs_sample_probs(gs_ctx *ctx, const double *scores, int s_loc, int64_t n, double *p_out,
                    int loc, double *total_out);
int gs_cumsum_ordered(gs_ctx *ctx, const double *p, int p_loc, int64_t n, double *out, int loc);

/* ---- symmetric random baseline: random.py:14-52 ----------------------------
 * gs_undirected_ids (precompute_random_scores, random.py:23-30): for column i,
 * inverse[i] = the rank of key_i = min(src, dst) * (n + 1) + max(src, dst) among
 * the distinct keys in ascending order, i.e. np.unique(keys, return_inverse=True)[1];
 * *n_undirected = the number of distinct keys (random.py:30).  src / dst at loc,
 * inverse at inv_loc (GS_HOST or GS_DEVICE).  *status: 0 = written; 1 = the input
 * is outside the device contract (an id outside [0, n), n < 1, n >= 2^31 or
 * E < 1) and nothing was written: the caller makes the reference's own calls, so
 * odd inputs behave as NumPy does (the ValueError of inverse_idx.max() on an empty
 * graph included).  One wait for the host, for the status and the count.  The
 * scores of random.py:31-32, default_rng(seed).random(n_undirected), are
 * gs_pcg64_doubles at offset 0 of the fresh generator's state.
 * gs_random_mask (random_sparsify, random.py:45-49): keep_undir = the n_keep
 * highest of the m scores on gs_topk_mask's keys and stable tie rule (n_keep >= m
 * keeps all, as argsort[-n_keep:] does; n_keep < 1 is GS_EINVAL: the caller passes
 * max(1, int(m * r)), random.py:46), held in the context; then mask[i] =
 * keep_undir[inverse[i]], i < E, with NumPy's index rule: an entry in [-m, 0)
 * wraps, any other entry outside [0, m) is counted in *n_bad (the mask is then
 * unspecified; the reference raises IndexError).  cut / n_beyond / n_tied as
 * gs_topk_mask returns them: 0 < n_keep - n_beyond < n_tied means np.argsort's
 * own order decides inside the tie block. */
int gs_undirected_ids(gs_ctx *ctx, int64_t n, int64_t E, const int64_t *src, const int64_t *dst,
                      int loc, int64_t *inverse, int inv_loc, int64_t *n_undirected,
                      int32_t *status);
int gs_random_mask(gs_ctx *ctx, const double *scores, int s_loc, int64_t m, int64_t n_keep,
                   const int64_t *inverse, int i_loc, int64_t E, uint8_t *mask, int m_loc,
                   double *cut, int64_t *n_beyond, int64_t *n_tied, int64_t *n_bad);

/* ---- maximum spanning forest under per-column scores ------------------------
 * The columns are the E columns of (src, dst), scores[i] belongs to column i
 * (nscores >= E).  Column i is better than column j when (key(score), index) is
 * lexicographically larger -- keep_lowest: smaller -- with gs_topk_mask's keys
 * (-0.0 == +0.0, NaN the largest) and its stable tie rule: a strict total order.
 * F = the columns Kruskal's walk, best first, adds because they join two components
 * of the undirected graph on n nodes; self-loop columns never do.  F is unique and
 * |F| = n - c, c = the components of that graph (isolated nodes count).
 * expand == 0: mask[i] = 1 on F.  expand != 0: mask[i] = 1 on every column whose
 * unordered pair {src, dst} is the pair of a column of F (the reverse direction
 * and duplicates), through gs_undirected_ids.
 * labels (optional, int32[n] at l_loc): one representative node per component.
 * *n_forest = |F|, *n_marked = mask bytes set, *rounds = Boruvka rounds that added a
 * column (<= ceil(log2 n)).  The host waits once per round.  E == 0: an empty mask.
 * GS_EINVAL: an id outside [0, n), nscores < E, n < 1.  GS_EUNSUPPORTED: n >= 2^31.
 * The result is the same bytes on every run. */
int gs_spanning_forest(gs_ctx *ctx, const double *scores, int s_loc, int64_t nscores,
                       const int64_t *src, const int64_t *dst, int e_loc, int64_t E, int64_t n,
                       int keep_lowest, int expand, uint8_t *mask, int m_loc, int32_t *labels,
                       int l_loc, int64_t *n_forest, int64_t *n_marked, int32_t *rounds);

/* ---- spectral sparsification by effective-resistance sampling ----------------
 * Spielman-Srivastava sampling over the undirected pairs of the E columns of
 * (src, dst); selection.spectral_sample is the definition and the result equals it
 * bit for bit.  inverse = gs_undirected_ids' ids, *m = their count.  Pair j takes the
 * score of its lowest column (scores[i] belongs to column i, nscores >= E); a loop
 * and a score that is NaN, +-inf or <= 0 give the rate 0, and p = rate / np.sum(rate)
 * (gs_sample_probs' blocked pairwise total).  rng is a Generator(PCG64) in the state
 * (state_hi/lo, inc_hi/lo).
 * method 0 (multinomial): cdf = cumsum(p) / cumsum(p)[-1]; draw j < q is double j of
 * the stream, searched side='right' (== rng.choice(m, q, True, p)); counts[j] = the
 * draws that landed on pair j, its weight counts / fl(q p).  *draws = q.
 * method 1 (independent): pair j is kept (counts 1) when double j of the stream is
 * < pk = min(1, fl(q p)), its weight 1 / pk; no cumsum.  *draws = m.
 * mask[i] = counts[inverse[i]] > 0 and weight[i] = the pair's weight (0 where
 * dropped), i < E; counts (optional, int64, room for E entries: the first *m are
 * written) and inverse (optional, int64[E]); each buffer at its own *_loc.
 * *n_kept_pairs = pairs with counts > 0, *max_count = the largest count,
 * *n_irregular = the non-loop pairs that do not have exactly two columns (one
 * direction only, duplicates: the weighted result would not be symmetric).
 * *status: 0 = written; 1 = degenerate input and nothing was written: ids outside
 * gs_undirected_ids' contract, nscores < E, a total that is not finite and positive,
 * q outside [1, 2^31) -- the caller evaluates selection.spectral_sample on the host,
 * so its exception surfaces.  GS_EINVAL: a method other than 0 / 1.
 * Integer atomics only: the outputs are the same bytes on every run. */
int gs_spectral_sample(gs_ctx *ctx, const double *scores, int s_loc, int64_t nscores,
                       const int64_t *src, const int64_t *dst, int loc, int64_t E, int64_t n,
                       int64_t q, int method, uint64_t state_hi, uint64_t state_lo,
                       uint64_t inc_hi, uint64_t inc_lo, uint8_t *mask, int m_loc, double *weight,
                       int w_loc, int64_t *counts, int c_loc, int64_t *inverse, int i_loc,
                       int64_t *m, int64_t *n_kept_pairs, int64_t *max_count,
                       int64_t *n_irregular, int64_t *draws, int32_t *status);

int gs_metric_backbone(gs_ctx *ctx, int64_t n, int64_t E, const int64_t *src,
                       const int64_t *dst, const double *w, int64_t nw, int loc, double eps,
                       uint8_t *keep, int keep_loc, int64_t *n_relax);
/* Part `part` of `nparts` of gs_metric_backbone (multi-GPU): keep
 * bytes of the columns (u, v) with max(u, v) % nparts == part -- both directions
 * of a pair in one part, ids as the library labels them (graphs without id
 * locality are relabeled by descending degree, so max(u, v) is the pair's
 * lower-degree endpoint) -- 0 elsewhere; the element-wise sum over parts equals
 * the whole keep mask. */
int gs_metric_backbone_part(gs_ctx *ctx, int64_t n, int64_t E, const int64_t *src,
                            const int64_t *dst, const double *w, int64_t nw, int loc, double eps,
                            int part, int nparts, uint8_t *keep, int keep_loc, int64_t *n_relax);

/* The metric backbone in stages, for N ranks (metric_backbone.py:86-111
 * decided by sources split over the ranks).  Every rank calls the stages in order
 * with its own part / nparts and exchanges between them:
 *   gs_bb_begin        relabel, G, and the landmark searches l = part (mod nparts);
 *                      n_landmarks = K.  Exchange: the K x n landmark labels
 *                      (gs_bb_landmarks_io, element-wise MIN over ranks; +inf where
 *                      another rank searched) and the K completeness flags (MAX).
 *   gs_bb_certify      2-hop witness and certificates of this part's column range.
 *                      Exchange: the E column states (gs_bb_state_io, element-wise
 *                      MAX: 0 open, 1 keep, 2 prune; every rule is exact, so ranks
 *                      that decide a column decide it alike).
 *   gs_bb_plan         the sources with open columns (the same on every rank) and
 *                      nbatch, the search batches in their processing order.
 *   gs_bb_search       batches [b0, b1) (0 <= b0 <= b1 <= nbatch), this part's every
 *                      nparts-th one; exchange the states (MAX) after each range.
 *   gs_bb_finish       keep bytes of every column (state 1).
 * dir 0 copies the library's buffer out to D / complete / state, 1 copies it in;
 * loc: GS_HOST or GS_DEVICE.  With one part and one range this is gs_metric_backbone. */
int gs_bb_begin(gs_ctx *ctx, int64_t n, int64_t E, const int64_t *src, const int64_t *dst,
                const double *w, int64_t nw, int loc, double eps, int part, int nparts,
                int32_t *n_landmarks);
int gs_bb_landmarks_io(gs_ctx *ctx, double *D, int32_t *complete, int loc, int dir);
int gs_bb_certify(gs_ctx *ctx, int part, int nparts);
int gs_bb_state_io(gs_ctx *ctx, uint8_t *state, int loc, int dir);
int gs_bb_plan(gs_ctx *ctx, int64_t *nbatch);
int gs_bb_search(gs_ctx *ctx, int64_t b0, int64_t b1, int part, int nparts);
int gs_bb_finish(gs_ctx *ctx, uint8_t *keep, int keep_loc, int64_t *n_relax);
/* The numbers the stages above take for n nodes (E > 0; with E = 0 a run has K = 0) on
 * rank lpart of nranks, with the GSPARSE_BB_* variables as they are now: out = {K
 * landmarks, 1 when their searches spread over the device, workgroups per landmark of
 * that form (0: this rank has none), and for nsrc sources with open columns: sources
 * per workgroup S, threads per workgroup, nbatch = ceil(nsrc / S), slabs = workgroups
 * launched at most}.  Host code only: needs no context and no device. */
int gs_bb_geometry(int64_t n, int64_t nsrc, int32_t nranks, int32_t lpart, int64_t out[7]);

/* Decision classes of the metric backbone (a diagnostic: which exact rule decided each
 * column of metric_backbone.py:97-111's comparison).  gs_bb_classes(ctx, 1) makes the
 * following backbone runs on ctx record a class byte per column; gs_bb_class_counts
 * returns, for the last run, counts[k] = columns decided by class k on this rank
 * (ncounts >= GS_BB_WHY_CLASSES; counts[GS_BB_WHY_OPEN] = columns this rank left to
 * others) and, when why != NULL, the E class bytes (nwhy >= E, else GS_EINDEX;
 * why_loc: GS_HOST / GS_DEVICE); n_columns (may be NULL) = E of that run. */
enum {
    GS_BB_WHY_OPEN = 0,
    GS_BB_WHY_SELF,         /* self-loop: d(u, u) = 0 */
    GS_BB_WHY_ISOLATED,     /* an endpoint without edges in G: keep */
    GS_BB_WHY_DEG1,         /* an endpoint of degree 1 whose neighbour is the other: d = w_G */
    GS_BB_WHY_DIRECT,       /* w > fl(w_G(u, v) + eps): prune */
    GS_BB_WHY_LOCAL2,       /* local lower bound from both endpoints' least other edges: keep */
    GS_BB_WHY_LM_COMP,      /* a complete landmark search reaches one endpoint only: keep */
    GS_BB_WHY_LM_PRUNE,     /* landmark upper bound: prune */
    GS_BB_WHY_LM_KEEP,      /* landmark lower bound: keep */
    GS_BB_WHY_WITNESS,      /* 2-hop witness path: prune */
    GS_BB_WHY_LOCAL34,      /* 2- / 3- / 4-edge local lower bound: keep */
    GS_BB_WHY_SEARCH_PRUNE, /* the source row's bounded search: prune */
    GS_BB_WHY_SEARCH_KEEP,  /* the source row's bounded search: keep */
    GS_BB_WHY_REV_EXACT,    /* the reverse row's search, exact rule */
    GS_BB_WHY_REV_PRUNE,    /* the reverse row's search, upper bound: prune */
    GS_BB_WHY_REV_KEEP,     /* the reverse row's search, unreached within its bound: keep */
    GS_BB_WHY_MITM,         /* meet-in-the-middle certificate (GSPARSE_BB_MITM=1) */
    GS_BB_WHY_CLASSES
};
int gs_bb_classes(gs_ctx *ctx, int on);
int gs_bb_class_counts(gs_ctx *ctx, int64_t *counts, int ncounts, uint8_t *why, int64_t nwhy,
                       int why_loc, int64_t *n_columns);

/* Exact shortest-path distances for nq node pairs (qs[q], qt[q]) (host arrays;
 * out host) in the graph metric_backbone.py:70-79 builds from the columns
 * (src, dst, w): undirected, the columns with src < dst, weight the minimum
 * over duplicates; w == NULL: unit weights (hop counts); nw = entries of w
 * (nw < E: GS_EINDEX).  +inf when
 * unreachable; 0 when qs == qt.  Bit-identical to NetworkX Dijkstra's
 * left-fold path sums.  Replaces the nx.shortest_path_length calls of
 * verify_geodesic_preservation (metric_backbone.py:144-225) and
 * compute_geodesic_preservation (metrics.py:361-442). */
int gs_pair_distances(gs_ctx *ctx, int64_t n, int64_t E, const int64_t *src, const int64_t *dst,
                      const double *w, int64_t nw, int loc, int64_t nq, const int64_t *qs,
                      const int64_t *qt, double *out);

/* Exact effective resistance of the resident (symmetric) graph, one score per
 * CSR entry.  Replaces calculate_effective_resistance_scores (metrics.py:124-175:
 * dense pinv of L + 1e-10 I).  Computed as G_uu + G_vv - 2 G_uv with G the
 * inverse of the grounded Laplacian M (one ground node per connected
 * component, its row/column read as zero), G from a blocked fp64-MFMA Cholesky
 * M = L L^T and L^-1 (GSPARSE_XER_METHOD=ns: Newton-Schulz); max(., 1e-10) as
 * the reference clamps.  n <= 32768: the dense form; *iterations (may be NULL)
 * receives the number of 64-row blocks (Cholesky) or Newton-Schulz steps.
 * Above: gs_exact_er_sparse with cg_rtol = 1e-12 and cg_max_iter = 5000, and
 * *iterations receives its batch count.  GS_EUNSUPPORTED for a directed
 * adjacency or asymmetric weights. */
int gs_exact_er(gs_ctx *ctx, double *out, int out_loc, int32_t *iterations);
/* The same scores with no dense matrix, for a symmetric graph of any n: for
 * every node u that is not grounded the column g_u of G solves M g_u = e_u by
 * CG on the ungrounded rows, Jacobi-preconditioned (the weighted degrees;
 * stored diagonal entries are no part of L), to a relative residual cg_rtol
 * within cg_max_iter iterations.  The columns run B at a time (B a multiple of
 * 64 from n and the device, GSPARSE_XER_BATCH overrides; four n x B fp64 blocks
 * and O(n + nnz) of memory), each with its own recurrence and stopping test; a
 * converged batch leaves G_uu and, per CSR entry (u,v) with u < v, G_vu, and
 * entry (v,u) takes the score of (u,v): out[e] == out[tpos[e]] bit for bit.
 * Reductions are two-stage in a fixed order that depends on n alone: two calls,
 * and two batch widths, give the same bits.  GS_EINVAL for cg_rtol outside
 * (0, 1) or cg_max_iter < 1, GS_EUNSUPPORTED for a directed adjacency or
 * asymmetric weights, GS_ENOCONV when a batch stops at cg_max_iter with a
 * column still open: out is then left untouched.  *batches (converged batches)
 * and *cg_iterations (the columns' iterations, summed) are written in both
 * cases; each may be NULL. */
int gs_exact_er_sparse(gs_ctx *ctx, double *out, int out_loc, double cg_rtol,
                       int32_t cg_max_iter, int32_t *batches, int64_t *cg_iterations);
/* The sparse form's plan for an n-node graph on a device of cus compute units
 * (<= 0: 256), under GSPARSE_XER_BATCH as it is now (host code, no device):
 * out = B, the byte budget of the four blocks, the row chunks of its vector
 * passes and the rows per chunk (both functions of n alone). */
int gs_xer_sparse_plan(int64_t n, int32_t cus, int64_t out[4]);

/* ---- compute_topology_metrics (metrics.py:445-520) on the resident graph ----
 * The resident graph must be symmetric; the clustering and the counts expect
 * it self-loop-free (NetworkX drops v from its own neighbour set).
 *
 * |N(u) ∩ N(v)| per CSR entry (exact integers as float64). */
int gs_common_neighbors(gs_ctx *ctx, double *out, int out_loc);
/* nx.average_clustering in NetworkX's operation order (bit-identical):
 * c_v = 0 if t == 0 else t / (d (d - 1)), t = sum of the counts of v's entries,
 * summed left to right from 0 in node order, / n.  per_node (may be NULL,
 * location per_loc) receives c_v. */
int gs_clustering(gs_ctx *ctx, double *avg, double *per_node, int per_loc);
/* Connected components (nx.connected_components): labels[u] = smallest node id
 * of u's component (may be NULL), *count, *largest (size of the largest). */
int gs_components(gs_ctx *ctx, int32_t *labels, int labels_loc, int64_t *count,
                  int64_t *largest);
/* Algebraic connectivity (nx.algebraic_connectivity, weighted, unnormalised;
 * metrics.py:478-510) of a connected resident graph: 1 / lambda_max(L^+) on the
 * mean-free vectors (P = I - 11^T/n), by Lanczos with full reorthogonalisation
 * until the Ritz value changes by <= tol (relative) or max_iter (<= 500)
 * steps.  n <= 32768: the dense form, L^+ = P G P with G the grounded inverse of
 * L (fp64-MFMA Cholesky).  Above: gs_fiedler_sparse with cg_rtol = 1e-10 and
 * cg_max_iter = 5000.  GS_EINVAL if the graph is not connected. */
int gs_fiedler(gs_ctx *ctx, double tol, int32_t max_iter, double *value, int32_t *iterations);
/* The same value with no dense matrix, for a connected symmetric graph of any
 * n >= 2 (the reference's tracemin_lu, metrics.py:478-510, has no size limit
 * either): L^+ is applied by a CG solve of L y = P v_j on the mean-free
 * vectors, Jacobi-preconditioned (the weighted degrees; stored diagonal entries
 * are no part of L), to a relative residual cg_rtol within cg_max_iter
 * iterations per solve.  Reductions are two-stage in a fixed order: two calls
 * give the same bits.  GS_EINVAL for several components, GS_EUNSUPPORTED for a
 * directed adjacency, GS_ENOCONV when a solve stops at cg_max_iter or Lanczos
 * at max_iter unconverged: *value is then left untouched.  *iterations (outer
 * steps) and *cg_iterations (inner iterations of all solves) are written in
 * both cases; each may be NULL. */
int gs_fiedler_sparse(gs_ctx *ctx, double tol, int32_t max_iter, double cg_rtol,
                      int32_t cg_max_iter, double *value, int32_t *iterations,
                      int64_t *cg_iterations);

/* ---- how good a sparsifier is: the spectral bounds of H against G ----------
 * G is the resident graph (symmetric, connected, non-negative weights; stored
 * diagonal entries are no part of L_G, as in gs_fiedler_sparse).  H is a graph
 * on the same nodes whose support is a subset of G's: hw[e] is its weight on
 * CSR entry e of G (nhw == nnz entries in the order gs_graph_copy_csr returns,
 * hw_loc: GS_HOST / GS_DEVICE), 0 for a dropped entry; diagonal entries are
 * ignored.  The outputs are the extreme eigenvalues of L_H x = lambda L_G x
 * over the mean-free vectors,
 *   lambda_min = min x'L_H x / x'L_G x,  lambda_max = max x'L_H x / x'L_G x,
 * so H is a (1 +- eps) spectral approximation of G with
 * eps = max(lambda_max - 1, 1 - lambda_min); lambda_min = 0 exactly when H
 * disconnects what G connects.  Lanczos on L_G^+ L_H in the L_G inner product
 * with full reorthogonalisation, each step one CG solve with L_G
 * (Jacobi-preconditioned, relative residual cg_rtol within cg_max_iter
 * iterations), until the residual bounds beta_j |s_last| of both extreme Ritz
 * pairs are <= tol lambda_max, beta_j falls to the level of the solve's
 * accuracy (an invariant subspace), or max_iter (<= 500) steps.  Defaults of the
 * Python layer: tol 1e-9, max_iter 300, cg_rtol 1e-10, cg_max_iter 5000.
 * Reductions are two-stage in a fixed order: two calls give the same bits.
 * GS_EINVAL: nhw != nnz, several components, n < 2, max_iter outside [2, 500],
 * cg_rtol outside (0, 1), cg_max_iter < 1, tol <= 0, an hw entry that is
 * negative or not finite.  GS_EUNSUPPORTED: a directed adjacency, or
 * hw[e] != hw[tpos[e]] bitwise.  GS_ENOCONV when a solve stops at cg_max_iter
 * or Lanczos at max_iter unconverged: both outputs are then left untouched.
 * *iterations (Lanczos steps) and *cg_iterations (inner iterations of all
 * solves) are written in both cases; each output may be NULL. */
int gs_spectral_bounds(gs_ctx *ctx, const double *hw, int hw_loc, int64_t nhw, double tol,
                       int32_t max_iter, double cg_rtol, int32_t cg_max_iter,
                       double *lambda_min, double *lambda_max, int32_t *iterations,
                       int64_t *cg_iterations);

/* ---- cohesion: the k-truss decomposition of the resident graph -------------
 * On the simple undirected graph of the resident CSR pattern (symmetric;
 * diagonal entries take no part, the multiplicities in data are ignored):
 * sup(e) is the number of triangles through e, the k-truss is the largest
 * subgraph in which every edge lies in at least k - 2 triangles of that
 * subgraph, and the trussness t(e) is the largest k whose k-truss contains e.
 * Every edge has t >= 2, an edge in no triangle has t = 2, every edge of a
 * clique K_c that touches nothing else has t = c.
 *
 * out[e] (nnz values, out_loc: GS_HOST / GS_DEVICE) is the trussness of CSR
 * entry e as an exact integer in float64, 0 on diagonal entries, and
 * out[e] == out[tpos[e]].
 *
 * The layering is that of the level-synchronous peel (Kabir and Madduri's PKT).
 * The supports start as gs_common_neighbors' counts (less the stored diagonal
 * entries of the two ends).  For s = 0, 1, ...: the frontier is the alive
 * edges with sup <= s; they get trussness s + 2 and are removed, which takes
 * one off the support of every alive edge per triangle lost; the alive edges
 * whose support thereby reaches s form the next frontier of the SAME level (a
 * sub-round), until that is empty; s then moves to the smallest alive support.
 * *levels counts the levels with a non-empty frontier (= the distinct
 * trussness values), *rounds their sub-rounds summed, *max_truss the largest
 * trussness (0 for a graph with no off-diagonal entry): all three are
 * properties of the graph, the same on every run, as out is (integer atomics
 * only).  *host_waits counts the times the call waited on the stream for the
 * peel (the edge count, once per level, once per sub-round or per chain of
 * sub-rounds taken by the tail); it depends on GSPARSE_TRUSS_TAIL, read on
 * every call: a sub-round whose frontier has at most that many edges (default
 * 16, 0: never), and at most twice as many 64-entry steps over the shorter
 * neighbour lists of its edges, is run by a single workgroup that goes on with
 * the level's sub-rounds by itself while the frontier stays within both bounds.
 * Each counter may be NULL.  GS_EUNSUPPORTED for a directed adjacency or
 * nnz >= 2^31 - 1; nnz == 0 gives an empty result and zeros. */
int gs_trussness(gs_ctx *ctx, double *out, int out_loc, int64_t *max_truss,
                 int32_t *levels, int64_t *rounds, int64_t *host_waits);

/* ---- local sparsification: segment ranks and the local-filter score ----------
 * (L-Spar, Satuluri et al. SIGMOD'11; Local Degree / Local Similarity, Hamann et
 * al.; NetworKit's local filter.  Not in the reference; the NumPy specification
 * is gsparse/selection.py: local_filter_scores.)
 * The columns are the E columns of edge_index, scores[i] belongs to column i
 * (nscores >= E).  The segment of node u is the set of columns with src == u,
 * d_u its length; loops and duplicate columns are ordinary columns.  Column i is
 * better than column j when (key(score), index) is lexicographically larger --
 * keep_lowest: smaller -- with gs_topk_mask's keys (-0.0 == +0.0, NaN the
 * largest): gs_spanning_forest's strict total order.
 * gs_segment_rank: rank[i] (int32) = the better columns of i's own segment, 0 =
 * the node's best edge; deg[u] (int64[n], may be NULL) = d_u; *max_deg = the
 * largest d_u.  class_counts[0..ncounts): nodes per GS_SEGR_* class, by segment
 * length: SHORT (<= 64) one column per lane of a sub-wave group and a count of
 * the better ones, LDS (<= 8192) one workgroup ordering the staged keys in LDS,
 * STREAM radix sorts of the hubs' columns.  GSPARSE_SEGR_SHORT_MAX / _LDS_MAX
 * lower the limits, GSPARSE_SEGR_MODE=sort takes every segment through the
 * STREAM class; all three are read on every call and change class_counts only.
 * Ties are broken by the column index itself: the same bytes on every run, for a
 * sorted and an unsorted src.  One wait for the host.  GS_EINVAL for nscores <
 * E, a src outside [0, n) or n < 1; GS_EUNSUPPORTED for E >= 2^31.
 * gs_local_scores: the local-filter score of every column from those ranks.
 * x[i] = 0 for rank[i] == 0, else table[rank[i] + 1] / table[deg[src[i]]] -- one
 * IEEE divide; table[j] = log(max(j, 1)), j < ntable, computed by the caller
 * (NumPy's log: the device calls none), so node u keeps column i at exponent e,
 * rank + 1 <= d_u^e, exactly when x[i] <= e.  y = the minimum of x over the
 * columns of the unordered pair {src, dst} (gs_undirected_ids; an integer
 * atomicMin on the bit patterns: exact and run-independent), out[i] = 1 - y: a
 * value in [0, 1], 1 = some end's best edge, and out >= 1 - e is the mask of the
 * local sparsifier at exponent e.  *n_top = columns with out == 1.  GS_EINVAL for
 * ntable <= the degree of a column's source, a rank outside [0, d), an id outside
 * [0, n) or n < 1; GS_EUNSUPPORTED for n >= 2^31.  E == 0 writes nothing. */
enum { GS_SEGR_EMPTY = 0, GS_SEGR_SHORT, GS_SEGR_LDS, GS_SEGR_STREAM, GS_SEGR_CLASSES };
int gs_segment_rank(gs_ctx *ctx, const double *scores, int s_loc, int64_t nscores,
                    const int64_t *src, int src_loc, int64_t E, int64_t n, int keep_lowest,
                    int32_t *rank, int rank_loc, int64_t *deg, int deg_loc, int64_t *max_deg,
                    int64_t *class_counts, int ncounts);
int gs_local_scores(gs_ctx *ctx, const int32_t *rank, int r_loc, const int64_t *src,
                    const int64_t *dst, int e_loc, int64_t E, int64_t n, const int64_t *deg,
                    int d_loc, const double *table, int t_loc, int64_t ntable, double *out,
                    int out_loc, int64_t *n_top);

/* ---- the Simmelian backbone: ranked-neighbourhood overlap ---------------------
 * (Nick, Lee, Cunningham, Brandes, ASONAM 2013; NetworKit's Simmelian
 * sparsifiers.  Not in the reference; the NumPy specification is
 * gsparse/selection.py: simmelian_host, the literal definition
 * simmelian_bruteforce.)
 * On the simple undirected graph of the resident CSR pattern (symmetric;
 * diagonal entries take no part and score 0, the multiplicities are ignored):
 * t(u, w) is the number of triangles through {u, w}.  For an edge {u, v} the ego
 * u ranks N(u) \ {v} by t, ties sharing the best rank, 0-based:
 * rho(w) = #{x in N(u) \ {v} : t(u, x) > t(u, w)}, and P_k(u|v) holds the
 * neighbours of rank < k (a tie group enters whole), so the score is a property
 * of the graph and not of the node numbering.
 *   max_rank == 0   out = max over k >= 1 of |P_k(u|v) n P_k(v|u)| /
 *                   |P_k(u|v) u P_k(v|u)|, 0 without a common neighbour.  The
 *                   candidates -- one per distinct larger rank of a common
 *                   neighbour -- are compared exactly in int64 and the result is
 *                   one IEEE division: the specification's bits.
 *   max_rank >= 1   out = |P_k(u|v) n P_k(v|u)| at k = max_rank, an exact integer
 *                   (NetworKit's parametric form).
 * out[e] (nnz float64 values, out_loc: GS_HOST / GS_DEVICE), out[e] ==
 * out[tpos[e]].  *max_common = the most common neighbours of a pair,
 * *nonzero_pairs = the pairs u < v with one; class_counts[0..ncounts): pairs per
 * GS_SIM_* class, by the shorter of the two neighbour lists: WAVE (<= 64) one
 * common neighbour per lane, MID (<= 512) a wave with an LDS slice, LDS (<= 8192)
 * a workgroup ordering the ranks in LDS, STREAM a radix sort of the hubs' (pair,
 * rank).  GSPARSE_SIM_WAVE_MAX / _MID_MAX / _LDS_MAX lower the bounds; they are
 * read on every call and change class_counts only.  Integer atomics only: the
 * same bytes on every run.  Each counter may be NULL.  GS_EINVAL for max_rank <
 * 0; GS_EUNSUPPORTED for a directed adjacency or nnz >= 2^31 - 1; nnz == 0 gives
 * an empty result and zeros. */
enum { GS_SIM_WAVE = 0, GS_SIM_MID, GS_SIM_LDS, GS_SIM_STREAM, GS_SIM_CLASSES };
int gs_simmelian(gs_ctx *ctx, double *out, int out_loc, int64_t max_rank, int64_t *max_common,
                 int64_t *nonzero_pairs, int64_t *class_counts, int ncounts);

#ifdef __cplusplus
}
#endif
#endif /* GSPARSE_H */
