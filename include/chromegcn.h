/*
 * chromegcn.h -- C ABI of libchromegcn_hip.so: the MI355X (gfx950) implementation of
 * ChromeGCN's per-chromosome gated graph-convolution hot path.
 *
 * The reference (QData/ChromeGCN) has no FFI of its own: its boundary for this path is
 * the Python nn.Module surface.  Each entry point below names the
 * reference code it replaces (file:line relative to the reference repository root); the
 * Python host side in chromegcn_amd/ binds them with ctypes (INTEGRATION.md shows the
 * stub a reference maintainer would add).
 *
 * Conventions
 *   - Every pointer is a DEVICE pointer unless marked "host".  No torch types.
 *   - All work is enqueued on `stream` (a hipStream_t passed as void*; cgcn_layer_bwd may also use
 *     a caller-provided auxiliary stream); nothing here synchronises the host, allocates or frees
 *     device memory, or keeps a caller pointer after return.
 *     All entry points are therefore legal inside HIP-graph stream capture.
 *   - Return value: CGCN_OK (0) or a negative CGCN_ERR_* code; cgcn_strerror() names it.
 *   - Dense matrices are row-major fp32.  Node features are laid out [S, n, d]:
 *     S strands (S = 1: one call of ChromeGCN.forward; S = 2: the forward and the
 *     reverse-complement strand of finetune.py:41-42 sharing one pass over the graph),
 *     n nodes (windows of one chromosome), d features.  d must be 128 or 256.
 *   - A graph is a CSR triple: rowptr[n+1], col[nnz] (int32, columns sorted or not),
 *     val[nnz] fp32 or NULL meaning "all ones", plus an optional per-row scale
 *     row_scale[n] (NULL = 1).  The row-normalised adjacency of process_graph
 *     (utils/util_methods.py:146-180) is A = diag(row_scale) * Ahat with
 *     row_scale = 1/deg; 'hic', 'constant' and 'none' graphs have val == NULL,
 *     'both' graphs carry val in {1,2,3}.
 *   - The backward needs Ahat^T; (rowptr_t, col_t, val_t) is its CSR.  Hi-C graphs are
 *     symmetric (data/7create_graph_new.py:115-116) so callers pass the same arrays.
 *   - aux / aux_t (may be NULL): optional facts about the graph (cgcn_graph_aux below) that change speed, never
 *     results beyond fp32 re-association: a uint16 copy of the column indices and the length of the longest row.
 *   - Dropout (F.dropout of models/ChromeModels.py:42,50) is counter based: a mask bit is a pure
 *     function of rng_state = {seed, step counter} (uint64[2] in DEVICE memory), a stream id and
 *     the element index, so the backward regenerates the forward's mask.  Every kernel of one
 *     train step must see the same counter; cgcn_sgd_step or cgcn_adam_step (the last kernel of a step) advances it.
 */
#ifndef CHROMEGCN_H
#define CHROMEGCN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CGCN_OK 0
#define CGCN_ERR_BAD_ARG (-1)     /* null pointer, negative size, misaligned buffer      */
#define CGCN_ERR_UNSUPPORTED (-2) /* d not in {128,256}, S not in {1,2}, size overflow   */
#define CGCN_ERR_LAUNCH (-3)      /* hipGetLastError() != hipSuccess after a launch      */
#define CGCN_ERR_WORKSPACE (-4)   /* workspace too small (see cgcn_*_workspace_bytes)    */

#define CGCN_ABI_VERSION 26

typedef void *cgcn_stream_t; /* hipStream_t */

/*
 * Optional per-graph facts (HOST struct; the arrays it points to are device memory).  Pass NULL for none.
 *   col16       : the same column indices as uint16, for graphs with at most 65 536 columns (every chromosome at 1 kb
 *                 windows with peaks), or NULL.  The feature-sliced aggregation kernels re-read the index list once per
 *                 128-byte column slice; the 16-bit copy halves those bytes.  Used only with implicit values
 *                 (val == NULL); results are bit-identical.
 *   max_row_len : number of stored entries of the longest row (0 = unknown).  The reference keeps the top-K contacts of a
 *                 chromosome (data/7create_graph_new.py:93-104), so a few windows can have thousands of neighbours.  A
 *                 row is aggregated inside one workgroup by the fused forward (one CU's L1: ~65 us for 10 000
 *                 neighbours of 1 KiB); graphs whose longest row exceeds 2 048 entries therefore take the feature-sliced
 *                 route (8 ... 16 workgroups per row) at every table size.
 *   row_order   : a permutation of 0 .. n_rows-1 (int32, device), or NULL = natural order: the order in which the
 *                 feature-sliced kernels deal the rows to their 64-row tiles (position p -> tile p / 64, wave (p % 64) / 8;
 *                 a wave walks its 8 rows side by side until the longest is done).  The engine passes the rows of every
 *                 64-row group sorted by length (a wave's 8 rows are then about equally long, a tile still holds
 *                 neighbouring rows) and the groups heaviest first (tiles with hub rows start the launch).  Results are
 *                 independent of the order up to fp32 re-association of a row's sum (a wave chooses how to walk its rows
 *                 by their lengths).  Not checked: an array that is not a permutation leaves rows unwritten.
 *   band_halfwidth : w > 0 says the CSR is EXACTLY a band: row i holds the columns max(0, i - w) .. min(n - 1, i + w), each
 *                 once (process_graph's 'constant' branch, utils/util_methods.py:137-150: w = 7; the diagonal is the
 *                 added identity), with implicit unit values (val == NULL).  0 = not a band / unknown.  For w = 7 the
 *                 aggregation then runs as a sliding-window stream over the table (k_band_aggregate / k_bwd_band: every
 *                 row read once, no index list) instead of the CSR walk; same bits (same summation order).  Not checked:
 *                 a wrong hint gives the band's sums, not the CSR's.  ABI 21.
 *   bp_rowptr, bp_col, bp_col16, bp_row_order : the "band plus" decomposition of an explicit-value graph whose values are 1
 *                 or 2 with every 2 inside the +-7 band and every position of the band + I present (process_graph's 'both'
 *                 branch on a {0,1} Hi-C matrix, utils/util_methods.py:168-171), or all NULL.  (bp_rowptr, bp_col) is the
 *                 CSR (int32, device) of the UNIT entries that are not the band's own -- entries outside the band, and one
 *                 unit of each value-2 entry inside it -- so that  sum_j w_ij x_j = sum_{bp entries} x_j + sum_{|j-i|<=7} x_j.
 *                 bp_col16 / bp_row_order are what col16 / row_order are for the main CSR.  The feature-sliced kernels then
 *                 walk the bp CSR with implicit values and 16-bit indices and add the band + I half from a window of the
 *                 table staged once per workgroup in LDS ('both' at 'hic' speed); graphs that carry it take the
 *                 feature-sliced route at every table size.  Used only when val != NULL; results equal the merged CSR's
 *                 up to fp32 re-association of a row's sum.  Not checked.  ABI 21.
 * For the backward (aux_t) all of them describe the CSR of Ahat^T.
 */
typedef struct cgcn_graph_aux {
  const uint16_t *col16;
  const int32_t *row_order;
  int32_t max_row_len;
  int32_t band_halfwidth;
  const int32_t *bp_rowptr;
  const int32_t *bp_col;
  const uint16_t *bp_col16;
  const int32_t *bp_row_order;
} cgcn_graph_aux;

/* ABI version of the loaded library (compare with CGCN_ABI_VERSION). */
int cgcn_abi_version(void);

/* Static string for an error code.  Never NULL. */
const char *cgcn_strerror(int code);

/*
 * Y[s,i,:] = row_scale[i] * sum_{k in row i} val[k] * X[s, col[k], :]
 * Unfused sparse aggregation.  Replaces torch.spmm(adj, support), models/SubLayers.py:46.
 * X, Y: [S, n_cols, d] and [S, n_rows, d]; X and Y must not alias.
 * d: any multiple of 4 up to 4096 (GraphConvolution takes arbitrary in/out widths, models/SubLayers.py:8-12);
 * d = 128 / 256 run tuned kernels.  The fused gated layer below needs d in {128, 256}.
 */
int cgcn_spmm(cgcn_stream_t stream, int n_rows, int n_cols, int S, int d,
              const int32_t *rowptr, const int32_t *col, const float *val, const float *row_scale,
              const float *X, float *Y, const cgcn_graph_aux *aux);

/*
 * One gated graph-convolution layer, forward (one fused launch; or two -- a feature-sliced aggregation into H and a
 * row-local launch on it -- when H is wanted and the feature table S*n*d*4 is too large for the L2s; same results):
 *     H  = diag(row_scale) Ahat X          (aggregation)
 *     U  = H W + b                          (models/SubLayers.py:43-50; the reference
 *                                            computes A (X W) + b -- same value up to fp32
 *                                            re-association)
 *     Z  = tanh(U)                          (models/ChromeModels.py:38 / :44)
 *     g  = sigmoid(Z . wg + cg)             (models/ChromeModels.py:39 / :45, nn.Linear(d,1))
 *     Xn = (1 - g) X + g Z                  (models/ChromeModels.py:40 / :46)
 * X, Xn, Z, H: [S,n,d].  gate: [S,n].  W: [d,d] stored in x out (GraphConvolution.weight).
 * b, wg: [d].  cg: [1] (device).  Z and H may be NULL for inference (they are what the
 * backward needs).  Xn must not alias X.
 * dropout_p > 0 additionally applies the inter-layer dropout of models/ChromeModels.py:42 to Xn
 * (Xn <- mask * Xn / (1-p), mask from (rng_state, stream_id)); pass 0 / NULL / 0 for none.
 * H_in (may be NULL): a previously computed H = diag(row_scale) Ahat X for this X and graph (H does not
 * depend on the layer's weights).  When given, the gather is skipped and H_in is streamed instead; H is
 * then not written (pass H = NULL, the saved tensor for the backward is H_in itself).
 * colstats (may be NULL) / colstats_rows: the first stage of the classifier head's BatchNorm batch statistics
 * (models/ChromeModels.py:58-59, nn.BatchNorm1d in training mode) of relu(Xn), taken while the tile is on chip, in the form
 * cgcn_layer_fwd_colstats_plan planned: colstats_rows = the plan's *rows_per_tile, colstats = a buffer of the plan's tile
 * count x [S][d][2] floats.  Hand (colstats, tiles, colstats_rows) to cgcn_head_train as col_stats.
 *   colstats_rows > 0 (RECORDS): per tile of colstats_rows nodes and (strand, column) the mean and the sum of squared
 *     deviations.  colstats_rows must be a multiple of 16 / S; more than 16 / S nodes per record (merged records) are
 *     produced by the two-launch route only and need H or H_in (CGCN_ERR_BAD_ARG otherwise).
 *   colstats_rows = -1 (CGCN_COLSTATS_ROWS_ACCUMULATE): the buffer holds 64-bit fixed-point integer totals (see the plan);
 *     this call zeroes them in its aggregation launch, so it takes the two-launch route: needs H or H_in, n >= 2, an 8-byte
 *     aligned buffer.
 *   colstats_rows = -2 (CGCN_COLSTATS_ROWS_ZERO_ONLY): this call produces NO statistics; its first launch zeroes the totals
 *     in `colstats` for a LATER call of the same step (the previous layer's forward prepares the last layer's buffer) ...
 *   colstats_rows = -3 (CGCN_COLSTATS_ROWS_ACCUMULATE_ZEROED): ... which then accumulates into them on ANY route, the fused
 *     kernel included (tables below the two-launch size keep their one-launch forward).  Hand the buffer to cgcn_head_train
 *     with col_stats_rows = -1 either way.
 * The mode is an argument of the call (ABI v24): nothing about it is read from process state.
 */
int cgcn_layer_fwd(cgcn_stream_t stream, int n, int S, int d,
                   const int32_t *rowptr, const int32_t *col, const float *val, const float *row_scale,
                   const float *X, const float *W, const float *b, const float *wg, const float *cg,
                   float *Xn, float *Z, float *H, float *gate,
                   float dropout_p, const unsigned long long *rng_state, unsigned int stream_id,
                   const float *H_in, float *colstats, int colstats_rows, const cgcn_graph_aux *aux);

/* Column-statistics modes of cgcn_layer_fwd / cgcn_head_train (cgcn_layer_fwd_colstats_plan's `mode`) ... */
#define CGCN_COLSTATS_RECORDS 0
#define CGCN_COLSTATS_ACCUMULATE 1
/* ... and the special values of colstats_rows (above). */
#define CGCN_COLSTATS_ROWS_ACCUMULATE (-1)
#define CGCN_COLSTATS_ROWS_ZERO_ONLY (-2)
#define CGCN_COLSTATS_ROWS_ACCUMULATE_ZEROED (-3)

/* What to allocate for the column statistics of cgcn_layer_fwd(n, S, d) in `mode`: returns the number of tiles ([S][d][2]
 * floats each; 0 = unsupported shape or mode), *rows_per_tile = the value to pass as colstats_rows / col_stats_rows.
 * CGCN_COLSTATS_RECORDS: *rows_per_tile = nodes per record (the last one may be shorter): 16 / S on tables that take the
 *   fused route, a multiple of it (one record per row-local workgroup) on tables that take the two-launch route.
 * CGCN_COLSTATS_ACCUMULATE (n >= 2; falls back to records for n < 2): *rows_per_tile = -1 -- the buffer is used as 64-bit
 *   integer fixed-point totals of sum relu(Xn) and sum relu(Xn)^2 per (strand, column), zeroed and added to inside
 *   cgcn_layer_fwd (order-independent, so bit-reproducible); cgcn_head_train, handed the same (buffer, tiles, -1), derives
 *   the BatchNorm statistics from the totals inside its main kernel and launches no finalize kernel; it also leaves the
 *   BatchNorm-BACKWARD column sums as integer totals in the same buffer (and writes the loss from a ticketed total) instead
 *   of launching a finish kernel: the cgcn_head_grad handed to cgcn_layer_bwd must then carry stat_acc = that buffer.
 *   Range of the fixed point (32 fraction bits): sum relu(Xn)^2 < 2.1e9 per column (rms |Xn| < 265 at n = 30 000); beyond
 *   it the statistics -- and the loss -- come out NaN (loudly wrong, never silently wrapped).  The caller decides per call
 *   from what it knows about its inputs: chromegcn_amd's engine bounds |Xn| by the input features per chromosome
 *   (finetune.GCNStage), its module-level entry points default to records. */
int cgcn_layer_fwd_colstats_plan(int n, int S, int d, int mode, int *rows_per_tile);

/* Test / tuning hook: feature-table size in bytes from which cgcn_layer_fwd takes the two-launch route when H is
 * given (0 = always, negative = restore the built-in default).  Process-wide. */
void cgcn_debug_set_fwd_split_bytes(long long bytes);

/* Measurement hook: how the dense fp32 products of the row-local kernels are formed.  CGCN_PRODUCTS_SPLIT (default): six
 * bf16 MFMA partial products of an EXACT three-way split of every fp32 operand (x = h + m + l, 8 + 8 + 8 significant
 * bits), fp32 accumulators -- fp32 arithmetic on the bf16 matrix cores, measured MORE accurate against float64 than the
 * chain (it rounds 8 times where the chain rounds K / 4 times; profiles/r06_bf16x6_probe.txt).  CGCN_PRODUCTS_FP32_CHAIN:
 * v_mfma_f32_16x16x4_f32, the form of rounds 1-5.  The two differ in the last bits.  Process-wide; initial value from the
 * environment (CGCN_PRODUCTS=fp32 | split); any other argument restores that initial value. */
#define CGCN_PRODUCTS_FP32_CHAIN 0
#define CGCN_PRODUCTS_SPLIT 1
void cgcn_debug_set_products(int mode);
int cgcn_debug_get_products(void);

/* Which kernels a call WOULD launch, so that a profiler prices the kernel that actually runs (bench.py's roofline);
 * nothing is launched, no GPU is needed.
 *   cgcn_debug_layer_fwd_route: the training forward (H given, no H_in) on this graph with column statistics as planned
 *     (colstats_rows as for cgcn_layer_fwd; 0 = none), under the current split threshold: 0 = the fused k_layer_fwd,
 *     1 = k_aggregate_sliced + k_layer_dense / k_layer_dense256 (large tables, hub-heavy graphs, accumulate mode),
 *     2 = k_band_aggregate + the row-local kernel (band graphs: cgcn_graph_aux::band_halfwidth; their backward's last
 *     launch is k_bwd_band instead of k_bwd_sliced).
 *   cgcn_debug_layer_bwd_route: the row-local launch of cgcn_layer_bwd: 0 = k_bwd_rowlocal256s (d = 256: four column-slab
 *     workgroups per range of 32-row tiles, both dense products in the launch; ABI <= 20: k_bwd_rowlocal256 + a second
 *     launch for dHs), 2 = k_bwd_rowlocal_ring (d = 128: row / matrix wave teams over a flag-synchronised LDS ring).
 *     (1 was the 48-row-tile kernel of ABI <= 18: no longer returned.)
 * Negative = error code (unsupported shape). */
int cgcn_debug_layer_fwd_route(int n, int S, int d, const cgcn_graph_aux *aux, int colstats_rows);
int cgcn_debug_layer_bwd_route(int n, int S, int d);

/*
 * State the fused head's backward leaves for the LAST gated layer's backward (cgcn_head_bwd with
 * dX == NULL fills dym / bnc inside its workspace; cgcn_head_workspace_layout gives their offsets).
 * With it, cgcn_layer_bwd recomputes dL/dXn per row (BatchNorm backward, ReLU mask, dropout mask)
 * instead of reading it: one launch and one [S,n,d] round trip less.
 */
typedef struct cgcn_head_grad {
  const float *dym;         /* [n,d]    */
  const float *bnc;         /* [S,2,d]  */
  const float *save_mean;   /* [S,d]    */
  const float *save_invstd; /* [S,d]    */
  const float *bn_w;        /* [d]      */
  float dropout_p;          /* head dropout probability (0 = none) */
  const unsigned long long *rng_state;
  /* in deferred mode cgcn_head_bwd leaves the second stage of dW_out / db_out to cgcn_layer_bwd, which runs it in
   * extra workgroups of its row-local kernel: */
  const float *part;        /* partials region of the head workspace (cgcn_head_workspace_layout) */
  int n_partials;           /* cgcn_head_bwd_partials(n) */
  int C;
  float *dW_out;            /* [C,d] */
  float *db_out;            /* [C]   */
  int accumulate;
  const float *dloss;       /* [1] upstream d loss when the workspace came from cgcn_head_train (whose results are for
                               d loss = 1); NULL when it came from cgcn_head_bwd with dpred (already scaled) */
  float *dbn_w;             /* [d] both set when the workspace came from cgcn_head_train: d(bn weight) / d(bn bias) */
  float *dbn_b;             /* [d] are then finished here as well (same accumulate flag); NULL after cgcn_head_bwd  */
  const void *stat_acc;     /* ABI v23: NULL, or -- when cgcn_head_train ran in accumulate mode (col_stats_rows = -1) -- the
                               SAME col_stats buffer: its backward block holds the BatchNorm-backward column sums as integer
                               totals and `bnc` is not read (cgcn_head_train launched no finish kernel to fill it) */
} cgcn_head_grad;

/*
 * Optional: the optimizer step of utils/util_methods.py:14-19's SGD (optimizer.step(), finetune.py:49) fused into
 * the LAST cgcn_layer_bwd call of a train step -- the first layer's backward, whose gather launch (dX != NULL) or
 * partial-sum launch (dX == NULL) finishes this layer's parameter sums in slab workgroups.  Those workgroups then apply
 * the update to the elements they have just finished, and further extra workgroups update every other element of
 * the flat arenas (their gradients were finished by earlier launches of the step): no cgcn_sgd_step launch.
 * param / grad / momentum_buf: flat fp32 arenas of `count` elements in which every parameter, its gradient and its
 * momentum buffer sit at the SAME offset; dW, db, dwg, dcg of this call must point into `grad`.  Semantics and the
 * rng_state counter advance are those of cgcn_sgd_step.  Needs n > 0, accumulate == 0, aux_stream == NULL, and -- when
 * dX is produced -- in_dropout_p == 0: the step advances the dropout counter inside the same launch that would read
 * it for the input-dropout mask (the first layer's input is never a dropped tensor: models/ChromeModels.py:37-42).
 */
typedef struct cgcn_sgd_fuse {
  float *param;
  const float *grad;
  float *momentum_buf;      /* NULL iff momentum == 0 */
  long long count;
  float lr, momentum, weight_decay, grad_scale;
  int nesterov;
  unsigned long long *rng_state;   /* may be NULL */
} cgcn_sgd_fuse;

/* Bytes of scratch cgcn_layer_bwd needs for (n, S, d).  0 on unsupported shapes. */
size_t cgcn_layer_bwd_workspace_bytes(int n, int S, int d);

/*
 * Backward of cgcn_layer_fwd (what autograd derives for models/ChromeModels.py:37-40 /
 * :43-46; math in SURVEY.md Appendix A).  Given dXn = dL/dXn [S,n,d] and optionally
 * dgate = dL/dgate [S,n] (NULL = 0):
 *     gamma = g (1-g) (sum_k dXn (Z - X) + dgate)
 *     dU    = (g dXn + gamma wg^T) (1 - Z^2)
 *     db = sum_rows dU,  dwg = sum_rows gamma Z,  dcg = sum gamma,  dW = H^T dU
 *     dHs   = diag(row_scale) dU W^T        (dL/dH, pre-scaled)
 *     dX    = (1-g) dXn + Ahat^T dHs
 * dX: [S,n,d], must not alias dXn; NULL = parameter gradients only (the gather over Ahat^T is skipped:
 * use it for the first layer when nobody needs d loss / d features).  dW [d,d], db [d], dwg [d], dcg [1] are overwritten
 * when accumulate == 0 and added to when accumulate != 0.  dHs is a [S,n,d] output (the gather's operand; also
 * the adjacency-saliency operand: dL/dA_ij = <dHs_i, X_j>, see cgcn_sddmm); it may be NULL when dX is NULL (then it
 * is not computed) and must not alias dX.  Sums over rows are two-stage and deterministic
 * (no float atomics): results are bit-reproducible run to run.
 * in_dropout_p > 0: X was produced by a layer that applied dropout (in_stream_id = that layer's
 * stream_id); dX is then the gradient w.r.t. the pre-dropout tensor (mask / (1-p) applied).
 * Exactly one of dXn and head must be non-NULL (head: see cgcn_head_grad).
 * aux_stream (may be NULL): a second stream on which the partial-sum reduction runs concurrently with the
 * gather kernel; forked from and joined back into `stream` with events inside this call.
 * sgd (may be NULL): see cgcn_sgd_fuse.
 */
int cgcn_layer_bwd(cgcn_stream_t stream, int n, int S, int d,
                   const int32_t *rowptr_t, const int32_t *col_t, const float *val_t, const float *row_scale,
                   const float *X, const float *Z, const float *H, const float *gate,
                   const float *W, const float *wg,
                   const float *dXn, const float *dgate,
                   float *dX, float *dHs, float *dW, float *db, float *dwg, float *dcg,
                   int accumulate, float in_dropout_p, const unsigned long long *rng_state,
                   unsigned int in_stream_id, const cgcn_head_grad *head,
                   void *workspace, size_t workspace_bytes, cgcn_stream_t aux_stream,
                   const cgcn_sgd_fuse *sgd, const cgcn_graph_aux *aux_t);

/*
 * Profiling hook: cgcn_layer_bwd one launch group at a time, so that each kernel can be bracketed with events on the
 * caller's stream (bench.py's per-kernel roofline).  phases: bit 0 = the row-local launch (k_bwd_rowlocal_ring / k_bwd_rowlocal256s),
 * bit 1 = the launch after it (k_bwd_sliced / k_bwd_band with the second-stage sums, or k_reduce_partials when dX ==
 * NULL).  phases == 3 is cgcn_layer_bwd without aux_stream / sgd.  A phase-2-only call works on the partials, dHs and
 * (head mode) dL/dXn an earlier phase-1 call left in workspace / dHs / dX.  Stateless like everything else here.
 */
int cgcn_debug_layer_bwd_phases(cgcn_stream_t stream, int n, int S, int d,
                                const int32_t *rowptr_t, const int32_t *col_t, const float *val_t, const float *row_scale,
                                const float *X, const float *Z, const float *H, const float *gate,
                                const float *W, const float *wg, const float *dXn, const float *dgate,
                                float *dX, float *dHs, float *dW, float *db, float *dwg, float *dcg,
                                int accumulate, float in_dropout_p, const unsigned long long *rng_state,
                                unsigned int in_stream_id, const cgcn_head_grad *head,
                                void *workspace, size_t workspace_bytes, int phases, const cgcn_graph_aux *aux_t);

/*
 * cgcn_layer_bwd with a COMPANION aggregation: one more, independent cgcn_spmm -- H = diag(row_scale) Ahat X of another
 * problem, cgcn_spmm's operands on a square operator -- enqueued by the same call.  The engine hands the first layer's
 * backward of chromosome c (the last launch of its train step) the first aggregation of chromosome c + 1, which reads the
 * graph and the input features only.  When the companion is the same instance of the feature-sliced kernels as the call's own
 * gather over Ahat^T -- equal S and d with S*d/32 <= 8, the same index width, both with or both without explicit values,
 * both or neither band-plus, and a problem for which cgcn_spmm takes the feature-sliced route -- its workgroups are a second
 * block range of that gather launch: one launch boundary fewer, nothing waits for anything inside the launch.  In every other
 * case (and without a gather launch: dX == NULL; with an aux_stream; on a band graph) the aggregation is launched on its own
 * right behind.  Either way H holds, bit for bit, what cgcn_spmm(stream, n, n, S, d, ..., X, H, aux) gives, and every other
 * output is cgcn_layer_bwd's.  companion == NULL: exactly cgcn_layer_bwd.
 * CGCN_ERR_BAD_ARG / CGCN_ERR_UNSUPPORTED as cgcn_spmm for the companion's operands, and CGCN_ERR_BAD_ARG when companion->H
 * is one of this call's own operands; nothing is launched then.  Additions to ABI 26: CGCN_ABI_VERSION stays 26, nothing
 * above changes.
 * cgcn_debug_layer_bwd_co_route: 1 when that companion would ride in the gather launch of such a call on `stream` alone
 * (have_dX: dX != NULL), 0 when it would be launched on its own, < 0: an error code.
 */
typedef struct cgcn_spmm_job {
  int n, S, d;
  const int32_t *rowptr;
  const int32_t *col;
  const float *val;         /* NULL = implicit unit values */
  const float *row_scale;   /* NULL = 1 */
  const float *X;           /* [S, n, d] */
  float *H;                 /* [S, n, d], written */
  const cgcn_graph_aux *aux;
} cgcn_spmm_job;

int cgcn_layer_bwd_co(cgcn_stream_t stream, int n, int S, int d,
                      const int32_t *rowptr_t, const int32_t *col_t, const float *val_t, const float *row_scale,
                      const float *X, const float *Z, const float *H, const float *gate,
                      const float *W, const float *wg,
                      const float *dXn, const float *dgate,
                      float *dX, float *dHs, float *dW, float *db, float *dwg, float *dcg,
                      int accumulate, float in_dropout_p, const unsigned long long *rng_state,
                      unsigned int in_stream_id, const cgcn_head_grad *head,
                      void *workspace, size_t workspace_bytes, cgcn_stream_t aux_stream,
                      const cgcn_sgd_fuse *sgd, const cgcn_graph_aux *aux_t, const cgcn_spmm_job *companion);

int cgcn_debug_layer_bwd_co_route(int n, int S, int d, const int32_t *rowptr_t, const int32_t *col_t, const float *val_t,
                                  int have_dX, const cgcn_graph_aux *aux_t, const cgcn_spmm_job *companion);

/* Bytes of scratch cgcn_head_fwd / cgcn_head_bwd need for (n, S, d, C).  0 on unsupported shapes. */
size_t cgcn_head_workspace_bytes(int n, int S, int d, int C);

/* Byte offsets, inside that workspace, of the dym [n,d], bnc [S,2,d] and per-workgroup partials regions
 * cgcn_head_bwd fills (host pointers; see cgcn_head_grad), and the number of partial blocks. */
int cgcn_head_workspace_layout(int n, int S, int d, int C, size_t *dym_offset, size_t *bnc_offset,
                               size_t *part_offset);
int cgcn_head_bwd_partials(int n);

/*
 * Classifier head + loss of the GCN-stage step, fused (models/ChromeModels.py:48-51 applied to each
 * strand, then finetune.py:43,45,52):
 *     y_s   = dropout(BatchNorm1d(relu(X_s)))     batch statistics over the n nodes when training
 *     pred  = mean_s (y_s W_out^T + b_out)        computed as (mean_s y_s) W_out^T + b_out
 *     loss  = mean over n*C of BCE-with-logits(pred, target);   probs = sigmoid(pred)
 * X: [S,n,d].  bn_w, bn_b, run_mean, run_var: [d]; num_batches_tracked: int64[1] or NULL.  W_out: [C,d],
 * b_out: [C], target: [n,C] (0/1 floats).  C <= 256 (the reference takes C from the data, main.py:35; the training
 * kernels walk the labels in passes of 128).
 * training != 0: batch statistics, running statistics updated once per strand in strand order (what two
 *   successive ChromeGCN.forward calls do), num_batches_tracked += S, dropout with probability dropout_p
 *   driven by rng_state (see Conventions; the head uses its own fixed stream id).  Outputs
 *   dpred = d loss / d pred [n,C] (may be NULL), save_mean / save_invstd [S,d].
 * training == 0: running statistics, no dropout; dpred, save_*, rng_state unused.
 * probs: [n,C]; loss: [1].
 */
int cgcn_head_fwd(cgcn_stream_t stream, int n, int S, int d, int C, const float *X, const float *bn_w,
                  const float *bn_b, float *run_mean, float *run_var, long long *num_batches_tracked,
                  float momentum, float eps, int training, const float *W_out, const float *b_out,
                  const float *target, float dropout_p, const unsigned long long *rng_state,
                  float *probs, float *loss, float *dpred, float *save_mean, float *save_invstd,
                  void *workspace, size_t workspace_bytes);

/*
 * The eval-mode classifier head of ONE ChromeGCN.forward call per strand (models/ChromeModels.py:48-51 with the module in
 * eval mode, what `model(x, adj)` returns as its second value): logits[s] = BatchNorm1d(relu(X[s])) W_out^T + b_out with
 * the RUNNING statistics, dropout off -- no strand mean, no sigmoid, no loss, nothing updated.  X: [S,n,d] -> logits: [S,n,C].
 */
int cgcn_head_logits(cgcn_stream_t stream, int n, int S, int d, int C, const float *X, const float *bn_w,
                     const float *bn_b, const float *run_mean, const float *run_var, float eps, const float *W_out,
                     const float *b_out, float *logits);

/*
 * Training-mode head forward fused with the tile-local half of its backward (one pass over X): same outputs as
 * cgcn_head_fwd(training = 1) -- probs, loss, save_mean / save_invstd, running-stat update -- and, left in
 * `workspace` for the backward, dym = d loss / d (mean_s y_s) and the per-workgroup partials of dW_out, db_out and
 * the BatchNorm sums, all for an upstream d loss of 1, plus bnc (the BatchNorm-backward column means, likewise for
 * d loss = 1).  The same workspace is then handed to cgcn_layer_bwd via cgcn_head_grad with .dloss, .dbn_w and .dbn_b
 * set: that call finishes every head gradient.  (cgcn_head_bwd with dpred == NULL and dX == NULL is accepted and
 * launches nothing.)  d loss / d pred never touches memory.
 * col_stats (may be NULL): the colstats output of the cgcn_layer_fwd call that produced X, with its tile count and
 * rows per tile (cgcn_layer_fwd_colstats_plan; rows = -1: accumulate mode, the integer totals); the head then skips its own first pass over X.
 */
int cgcn_head_train(cgcn_stream_t stream, int n, int S, int d, int C, const float *X, const float *bn_w,
                    const float *bn_b, float *run_mean, float *run_var, long long *num_batches_tracked,
                    float momentum, float eps, const float *W_out, const float *b_out, const float *target,
                    float dropout_p, const unsigned long long *rng_state, float *probs, float *loss,
                    float *save_mean, float *save_invstd, const float *col_stats, int col_stats_tiles,
                    int col_stats_rows, void *workspace, size_t workspace_bytes);

/*
 * Profiling hook: cgcn_head_train one launch group at a time.  phases: bit 0 = batch statistics (k_head_colstats unless
 * col_stats is given, k_head_bn_finalize -- this one updates the running statistics), bit 1 = k_head_fused (one launch
 * per pass of <= 128 labels), bit 2 = k_head_train_finish.  phases == 7 is cgcn_head_train.
 */
int cgcn_debug_head_train_phases(cgcn_stream_t stream, int n, int S, int d, int C, const float *X, const float *bn_w,
                                 const float *bn_b, float *run_mean, float *run_var, long long *num_batches_tracked,
                                 float momentum, float eps, const float *W_out, const float *b_out, const float *target,
                                 float dropout_p, const unsigned long long *rng_state, float *probs, float *loss,
                                 float *save_mean, float *save_invstd, const float *col_stats, int col_stats_tiles,
                                 int col_stats_rows, void *workspace, size_t workspace_bytes, int phases);

/*
 * Backward of cgcn_head_fwd (training mode).  dloss: [1] upstream gradient of the loss or NULL (= 1).
 * Outputs dX [S,n,d] and, overwritten (accumulate == 0) or added to (accumulate != 0): dW_out [C,d],
 * db_out [C], dbn_w [d], dbn_b [d].  With dX == NULL ("deferred mode") only dbn_w, dbn_b and the dym / bnc /
 * partials state are produced; dX, dW_out and db_out are then finished by cgcn_layer_bwd given a
 * cgcn_head_grad that points at this workspace.  dpred == NULL (with dX == NULL): the workspace comes from
 * cgcn_head_train and already holds dym and the partials.  rng_state: same contents as in the forward.  Deterministic.
 */
int cgcn_head_bwd(cgcn_stream_t stream, int n, int S, int d, int C, const float *X, const float *bn_w,
                  const float *bn_b, const float *save_mean, const float *save_invstd, const float *W_out,
                  const float *dpred, const float *dloss, float dropout_p, const unsigned long long *rng_state,
                  float *dX, float *dW_out, float *db_out, float *dbn_w, float *dbn_b, int accumulate,
                  void *workspace, size_t workspace_bytes);

/*
 * Sampled dense-dense product on the graph's sparsity pattern:
 *     out[k] = sum_s < A[s,i,:], B[s,col[k],:] >     for every stored entry k of row i.
 * With A = dL/dU and B = X W of one layer this is dL/dA_ij on the pattern, i.e. the adjacency saliency
 * of scripts/visualize.py:29-49 (which materialises a dense n x n gradient on the CPU).  A, B: [S,n,d].
 * accumulate != 0: out[k] += the product (the saliency sums one product per layer).
 */
int cgcn_sddmm(cgcn_stream_t stream, int n, int S, int d, const int32_t *rowptr, const int32_t *col,
               const float *A, const float *B, float *out, int accumulate);

/*
 * The row normalisation of that saliency, scripts/visualize.py:49-55, on the pattern and in the reference's order of
 * operations: v[k] = |val[k] * raw[k]| (val == NULL: ones), out[k] = (v[k] / s_i) / m_i with s_i = the sum of row i's v (1 where
 * it is 0) and m_i = the maximum of row i's quotients (1 where it is 0).  raw, out: [nnz]; out may alias raw.
 */
int cgcn_saliency_normalize(cgcn_stream_t stream, int n, const int32_t *rowptr, const float *val, const float *raw, float *out);

/* adj_type codes of the device-side normaliser: the branches of process_graph, utils/util_methods.py:148-174 */
#define CGCN_ADJ_HIC 0
#define CGCN_ADJ_CONSTANT 1
#define CGCN_ADJ_BOTH 2
#define CGCN_ADJ_NONE 3

/*
 * Device-side process_graph (utils/util_methods.py:146-180), step 1 of 2: per-row entry counts of
 * A-hat (row_counts[n]) and their exclusive prefix sum (rowptr_out[n+1]; rowptr_out[n] = nnz(A-hat),
 * which the caller reads back once to size col_out).  Input: canonical CSR (sorted columns, no
 * duplicates) of the raw Hi-C matrix, fp32 values or NULL = ones; ignored for CONSTANT / NONE.
 */
int cgcn_graph_count(cgcn_stream_t stream, int n, int adj_type, const int32_t *rowptr_in, const int32_t *col_in,
                     const float *val_in, int32_t *row_counts, int32_t *rowptr_out);

/*
 * Step 2: columns of A-hat (sorted), values (val_out; required for BOTH, optional/ignored otherwise: HIC,
 * CONSTANT and NONE graphs are all-ones), row_scale = fp32(1 / rowsum) with 1/0 -> 0.
 * symmetric_flag (int32[1], caller sets it to 1; may be NULL): cleared if A-hat != A-hat^T.
 */
int cgcn_graph_fill(cgcn_stream_t stream, int n, int adj_type, const int32_t *rowptr_in, const int32_t *col_in,
                    const float *val_in, const int32_t *rowptr_out, int32_t *col_out, float *val_out,
                    float *row_scale, int32_t *symmetric_flag);

/* Bytes of scratch cgcn_multilabel_metrics needs (sort buffers + rocPRIM temporary storage). */
size_t cgcn_metrics_workspace_bytes(long long n, int C);

/*
 * Per-label ranking metrics of the reference's compute_metrics (utils/evals.py:89-92, utils/metrics.py),
 * computed on the device from probs [n,C] and 0/1 targets [n,C]:
 *   out[0*C + c] AUROC (roc_auc_score; NaN when label c has a single class present)
 *   out[1*C + c] area under sklearn's precision_recall_curve by the trapezoid rule (utils/metrics.py:168-176)
 *   out[2*C + c] recall at the first curve point (from the low-threshold end) with FDR <= fdr_cutoff
 *                (utils/metrics.py:148-160, cutoff 0.5 there)
 *   out[3*C + c] average precision (mean over labels = mean_average_precision, utils/metrics.py:25-26)
 * Tied scores form one curve point, as in sklearn.  n*C < 2^31.
 */
int cgcn_multilabel_metrics(cgcn_stream_t stream, long long n, int C, const float *probs, const float *targets,
                            float fdr_cutoff, float *out, void *workspace, size_t workspace_bytes);

/*
 * The same metrics for NON-NEGATIVE scores -- probabilities, which is what the reference's compute_metrics is given
 * (finetune.py:52 stores F.sigmoid(pred); utils/evals.py:26): with the sign known a (score, target) pair is a 32-bit
 * key and the library sorts every label's list with its own segmented radix sort (4 passes of 8 bits over all labels
 * at once) instead of one device-wide sort of 64-bit keys; same `out`, same workspace size
 * (cgcn_metrics_workspace_bytes), same tie rule, bit-identical results.
 * bad: device int32[1]; set to 1 when a score was negative or NaN -- `out` is then unspecified and the caller repeats
 * the call with cgcn_multilabel_metrics (chromegcn_amd.metrics does; it reads `bad` with the results, no extra sync).
 */
int cgcn_multilabel_metrics_nonneg(cgcn_stream_t stream, long long n, int C, const float *probs, const float *targets,
                                   float fdr_cutoff, float *out, int32_t *bad, void *workspace, size_t workspace_bytes);

/*
 * torch.optim.SGD step on one flat fp32 buffer (utils/util_methods.py:14-19 builds
 * SGD(lr, momentum=0.9, weight_decay=1e-6); dampening 0):
 *     d = grad_scale * grad + weight_decay * param;  buf = momentum * buf + d;
 *     param -= lr * (nesterov ? d + momentum * buf : buf)
 * momentum_buf zero-initialised reproduces torch's first step (buf = d); may be NULL when momentum == 0.
 * grad_scale: 1, or 1/k when grad holds the all-reduced SUM of k ranks' gradients (multi-GPU step group).
 * rng_state (may be NULL): its step counter is advanced by one -- this is the last kernel of a train step.
 */
int cgcn_sgd_step(cgcn_stream_t stream, long long count, float *param, const float *grad, float *momentum_buf,
                  float lr, float momentum, float weight_decay, int nesterov, float grad_scale,
                  unsigned long long *rng_state);

/*
 * torch.optim.Adam step on flat fp32 buffers (utils/util_methods.py:14-16 builds Adam(betas=(0.9, 0.98), lr), the
 * reference's default optimizer; amsgrad = maximize = False, L2 weight decay as torch.optim.Adam, not AdamW):
 *     g = grad_scale * grad + weight_decay * param;  t = step + 1;
 *     exp_avg += (1 - beta1) * (g - exp_avg);  exp_avg_sq = beta2 * exp_avg_sq + (1 - beta2) * g * g;
 *     param -= (lr / bc1) * exp_avg / (sqrt(exp_avg_sq) / bc2s + eps)
 * with bc1 = 1 - beta1^t, bc2s = sqrt(1 - beta2^t) computed in double and rounded once to fp32.  ABI 26.
 * beta1 / beta2 are the fp32 values given: 1 - beta is formed from them (1 - 0.9f is 2.4e-7 off 0.1, torch rounds 0.1).
 * exp_avg / exp_avg_sq zero-initialised with step 0 reproduce torch's first step.  An element whose exp_avg is 0 keeps
 * its value (padding between parameters stays 0 even with eps == 0).
 * step: device float[n_step], one count per parameter (torch keeps a 0-d float32 device tensor per parameter for
 *     fused / capturable Adam); the launch reads step[0] and adds 1 to every entry exactly once.
 * ticket: device int32[1], zero before the first launch and left at 0 by every launch (the last workgroup to finish
 *     writes the new step counts and resets it).  One launch at a time per ticket: launches that share one must be
 *     ordered (same stream, or events).
 * param, grad, exp_avg, exp_avg_sq: 16-byte aligned, count elements each (count need not be a multiple of 4).
 * grad_scale: 1, or 1/k when grad holds the all-reduced SUM of k ranks' gradients (multi-GPU step group).
 * rng_state (may be NULL): its step counter is advanced by one -- this is the last kernel of a train step.
 * Rejected on the host, nothing launched: CGCN_ERR_BAD_ARG for count < 0, n_step < 1, a NULL step / ticket, a NULL
 * buffer when count > 0, a misaligned buffer, beta1 or beta2 outside [0, 1), eps < 0 (or NaN);
 * CGCN_ERR_UNSUPPORTED for count >= 2^31.
 */
int cgcn_adam_step(cgcn_stream_t stream, long long count, float *param, const float *grad, float *exp_avg,
                   float *exp_avg_sq, float *step, int n_step, int32_t *ticket, float lr, float beta1, float beta2,
                   float eps, float weight_decay, float grad_scale, unsigned long long *rng_state);

/*
 * Label-pair Hi-C edge ablation (scripts/visualize.py:79-119, the TF-TF interaction map; chromegcn_amd/ablation.py).
 * These six functions are additions to ABI 26: CGCN_ABI_VERSION stays 26, nothing above changes.
 * For labels (i, j) with positive rows P_c = {u : targets[u, c] != 0}: every stored entry (u, v) with u in P_i and
 * v in P_j is removed from A-hat (the self loop too), the touched rows renormalised (a row left empty stays zero), and
 *     M[i * C + j] = (base_i - abl_ij) / base_i,
 * base_i / abl_ij = mean over P_i of sigmoid((logit_fwd(u, i) + logit_rev(u, i)) / 2) on the full / ablated graph;
 * exactly 0 when the pair removes no stored entry.  S must be 2 (both strands), d 128 or 256, else
 * CGCN_ERR_UNSUPPORTED; NULL buffers and negative sizes are CGCN_ERR_BAD_ARG.  Every sum is in a fixed order.
 *
 * Set-up, once per call: label_bits uint32 [n][(C + 31) / 32] (bit c of row u: u in P_c); pos_lists int32 [C][n]
 * (pos_lists[c * n + k]: the k-th row of P_c, ascending); pos_ranks int32 [C][n] (k, or -1 outside P_c);
 * pos_counts int32 [C] (|P_c|).
 */
int cgcn_ablation_prepare(cgcn_stream_t stream, int n, int C, const float *targets, uint32_t *label_bits,
                          int32_t *pos_lists, int32_t *pos_ranks, int32_t *pos_counts);

/*
 * Bytes of the restricted route's workspace for n_inst = (column labels of a batch) x |P_i| row instances and
 * layers in {1, 2}, or 0 when unsupported: [X1: n_inst * S * d fp32][X2: the same, layers == 2][removed: n_inst int32],
 * each part starting at a 256-byte boundary.
 */
size_t cgcn_ablation_workspace_bytes(int n_inst, int S, int d, int layers);

/*
 * Restricted route, one gated layer for the instances (b, k) of row label i, b < n_cols, k < n_pos = |P_i|: row
 * u = pos_list[k] under the mask of column label cols[b].  X [S, n, d] is the unablated input of the layer; X_inst
 * (NULL for layer 1) the instances' ablated input [n_cols][n_pos][S][d], read for the neighbours v in P_i (pos_rank:
 * the [n] ranks of P_i) and for the row itself.  Kept neighbours only are gathered and scaled by 1 / kept sum (by the row's
 * own scale where nothing was removed or that sum is 0; a row that keeps nothing is exactly 0); then U = H W + b, Z = tanh U,
 * g = sigmoid(Z . wg + cg), X_out = (1 - g) X_u + g Z in fp32, [n_cols][n_pos][S][d].  removed (may be NULL):
 * int32 [n_cols][n_pos], the entries each instance's row lost.
 */
int cgcn_ablation_layer(cgcn_stream_t stream, int n, int S, int d, const int32_t *rowptr, const int32_t *col,
                        const float *val, const float *row_scale, const float *X, const float *X_inst, const float *W,
                        const float *b, const float *wg, const float *cg, const uint32_t *label_bits, int C,
                        const int32_t *pos_list, const int32_t *pos_rank, int n_pos, const int32_t *cols, int n_cols,
                        float *X_out, int32_t *removed);

/*
 * Restricted route, label i's eval head (ReLU, BatchNorm from the running statistics, W_out[i] . y + b_out[i] per
 * strand, strand mean, sigmoid) and the fixed-order mean over P_i.
 *   label < 0: base_c for every label c from the unablated last-layer output X [S, n, d] (pos_lists, pos_counts);
 *              NaN for an empty P_c.
 *   label = i: M[i * C + cols[b]] for b < n_cols from the instance rows X_inst [n_cols][n_pos][S][d], with base and
 *              the removed counts of cgcn_ablation_layer.
 */
int cgcn_ablation_head(cgcn_stream_t stream, int n, int S, int d, int C, const float *X, const float *X_inst,
                       const float *bn_w, const float *bn_b, const float *run_mean, const float *run_var, float eps,
                       const float *W_out, const float *b_out, const int32_t *pos_lists, const int32_t *pos_counts,
                       int label, int n_pos, const int32_t *cols, int n_cols, const int32_t *removed, float *base,
                       float *M);

/*
 * Composed route, the masked graph of pair (label_i, label_j) on the unchanged pattern: val_out[nnz] (val, or 1 when
 * NULL, with the removed entries 0), row_scale_out[n] (row_scale, or 1 when NULL, for untouched rows; 1 / kept sum for
 * touched ones, unchanged where that sum is 0, and 0 when nothing is kept) and removed (int32 [1]): the number of removed
 * entries.
 */
int cgcn_ablation_mask(cgcn_stream_t stream, int n, int C, const int32_t *rowptr, const int32_t *col, const float *val,
                       const float *row_scale, const uint32_t *label_bits, int label_i, int label_j, float *val_out,
                       float *row_scale_out, int32_t *removed);

/*
 * Composed route, mean over P_i of sigmoid of the strand-mean logits [S, n, C]: label < 0 writes base_c for every c;
 * label = i writes M[i * C + col_label] from base[i] and removed[0] (exactly 0 when it is 0).
 */
int cgcn_ablation_reduce(cgcn_stream_t stream, int n, int S, int C, const float *logits, const int32_t *pos_lists,
                         const int32_t *pos_counts, int label, int col_label, const int32_t *removed, float *base,
                         float *M);

/*
 * The top-K Hi-C contact graph of one chromosome from its raw contact records (data/7create_graph_new.py:51-120, :168;
 * chromegcn_amd/hic.py).  These three functions are additions to ABI 26: CGCN_ABI_VERSION stays 26, nothing above changes.
 *   pos1, pos2 int32 [M]: the two start positions of every record, in file order; count fp64 [M]: the observed value;
 *   norm fp64 [n_bins] or NULL: the normalisation vector, indexed by pos / resolution_bp (NaN and 0 read as +inf, and so
 *       does a bin outside the vector); window_start int32 [N], strictly increasing: the windows with peaks (a window's
 *       node index is its rank).
 * Rule: a record survives iff pos1 != pos2 and both occur in window_start; its value is count / (nv[b1] * nv[b2]) in fp64
 * (one multiply, one divide; count itself when norm is NULL); the K = hic_edges / 2 survivors that come first in a STABLE
 * descending sort by value are taken (ties at the threshold: file order; fewer than K survivors: all of them); every taken
 * record sets A[i, j] = A[j, i] = 1.  Result: canonical {0,1} CSR (sorted columns, no values, symmetric, no diagonal):
 * rowptr_out int32 [N + 1], col_out int32 [2 min(K, capacity)] of which the first nnz_out[0] (device int32 [1]) are written.
 * Not defined: two records with the same ordered (pos1, pos2), NaN values, 2 K >= 2^31.
 *
 * Two calls, because the buffers are sized by the survivor count S, which only the device knows: cgcn_hic_count leaves S
 * in n_survivors (device int64 [1]; it depends on the records and the windows only, not on norm or K); the caller reads it
 * once and hands it to cgcn_hic_build as `capacity` (any bound >= S is as good).  cgcn_hic_build writes S again; when it
 * exceeds `capacity` nothing is overrun and the graph is that of the first `capacity` survivors: repeat with a larger one.
 * All of it is enqueued on `stream`: no allocation, no synchronisation, nothing retained between calls.
 * CGCN_ERR_BAD_ARG: a negative size, a NULL buffer that would be read or written, norm with resolution_bp < 1;
 * CGCN_ERR_UNSUPPORTED: capacity or 2 K >= 2^31; CGCN_ERR_WORKSPACE: workspace_bytes below
 * cgcn_hic_workspace_bytes(M, N, capacity, K) (cgcn_hic_count: capacity = K = 0), which is 0 for unsupported sizes.
 */
size_t cgcn_hic_workspace_bytes(long long M, int N, long long capacity, long long K);

int cgcn_hic_count(cgcn_stream_t stream, long long M, const int32_t *pos1, const int32_t *pos2,
                   const int32_t *window_start, int N, void *workspace, size_t workspace_bytes, long long *n_survivors);

int cgcn_hic_build(cgcn_stream_t stream, long long M, const int32_t *pos1, const int32_t *pos2, const double *count,
                   const double *norm, long long n_bins, int resolution_bp, const int32_t *window_start, int N,
                   long long K, long long capacity, void *workspace, size_t workspace_bytes, int32_t *rowptr_out,
                   int32_t *col_out, int32_t *nnz_out, long long *n_survivors);

/*
 * The same graph from records COARSER than the windows (K562: 5 kb records, 1 kb windows; data/extras/upsample_hic.py:36-44,
 * data/create_data.py:47-55).  Additions to ABI 26 like the three functions above; nothing above changes.
 * window_bp divides resolution_bp, up = resolution_bp / window_bp, 1 <= up <= 8.
 * Rule: (1) the EXPANDED FILE of the records (pos1, pos2, count) is, for each record in file order, for a = 0 .. up - 1, for
 * b = 0 .. up - 1, the record (pos1 + a window_bp, pos2 + b window_bp, count); (2) the graph is the rule of cgcn_hic_build
 * applied to the expanded file with the same norm, resolution_bp, window_start and K: a child survives iff its two positions
 * differ and both occur in window_start; its value is count / (nv[b1] * nv[b2]) with the norm bins of the SOURCE record (all
 * up^2 children of a record share them and so its value); the stable descending top-K, ties in the order of the expanded file;
 * A[i, j] = A[j, i] = 1.  A record (p, p) yields the up^2 - up ordered pairs a != b, (p + a, p + b) and (p + b, p + a) both
 * counting against K.  Nothing is expanded in memory: the filter reads the 16 B of a source record and writes only the
 * surviving children.  Contract: pos1, pos2 multiples of resolution_bp (blocks of different records cannot collide); what the
 * rule above leaves undefined stays undefined.  up = 1 gives byte for byte what cgcn_hic_count / cgcn_hic_build give.
 *
 * n_window_bins: the extent of the window bitmap, (last window start) / window_bp + 1, which the host knows.  A position at or
 * beyond n_window_bins * window_bp is no window; a window start at or beyond it is the caller's error and is ignored (never an
 * out-of-bounds write).  window_start stays any strictly increasing vector: when a start is negative or no multiple of
 * window_bp the passes find the children by binary search instead of the bitmap, and the graph is the rule's all the same.
 *
 * Calls, sizes and conventions as for cgcn_hic_count / cgcn_hic_build: n_survivors and capacity count survivors of the
 * expanded file; on overflow the graph is that of the first `capacity` of them.  Enqueue only, no allocation, no sync.
 * CGCN_ERR_BAD_ARG: as above, and resolution_bp < 1, window_bp < 1, window_bp not dividing resolution_bp, n_window_bins < 0;
 * CGCN_ERR_UNSUPPORTED: as above, and up > 8, M up^2 >= 2^31; CGCN_ERR_WORKSPACE: workspace_bytes below
 * cgcn_hic_up_workspace_bytes(...) (cgcn_hic_count_up: capacity = K = 0), which is 0 for sizes the other two reject.
 */
size_t cgcn_hic_up_workspace_bytes(long long M, int N, long long capacity, long long K, int resolution_bp, int window_bp,
                                   long long n_window_bins);

int cgcn_hic_count_up(cgcn_stream_t stream, long long M, const int32_t *pos1, const int32_t *pos2,
                      const int32_t *window_start, int N, int resolution_bp, int window_bp, long long n_window_bins,
                      void *workspace, size_t workspace_bytes, long long *n_survivors);

int cgcn_hic_build_up(cgcn_stream_t stream, long long M, const int32_t *pos1, const int32_t *pos2, const double *count,
                      const double *norm, long long n_bins, int resolution_bp, int window_bp, long long n_window_bins,
                      const int32_t *window_start, int N, long long K, long long capacity, void *workspace,
                      size_t workspace_bytes, int32_t *rowptr_out, int32_t *col_out, int32_t *nnz_out,
                      long long *n_survivors);

/*
 * Distance-aware graphs (chromegcn_amd/hicdist.py).  These six functions are additions to ABI 26:
 * CGCN_ABI_VERSION stays 26, nothing above changes.
 *
 * The four *_dist functions are cgcn_hic_count / cgcn_hic_build / cgcn_hic_count_up / cgcn_hic_build_up with two more rules:
 *   min_distance_bp >= 0: a record takes part only if |pos1 - pos2| >= min_distance_bp (computed in 64 bits); with window_bp
 *       the test is on the SOURCE record, before it is expanded.  Everything else about survival stays, and n_survivors and
 *       capacity count what survives both rules.
 *   expected fp64 [n_expected] or NULL: the value becomes (count / (nv[b1] * nv[b2])) / ex[d], two fp64 divisions in that
 *       order, d = |pos1 / resolution_bp - pos2 / resolution_bp| (floor division; the source record's bins with window_bp),
 *       ex = expected with NaN, 0 and negative entries read as +inf, and so does a distance outside the vector.
 * min_distance_bp = 0 and expected = NULL give byte for byte what the functions above give.  Workspaces: those of
 * cgcn_hic_workspace_bytes / cgcn_hic_up_workspace_bytes.  CGCN_ERR_BAD_ARG also for min_distance_bp < 0, n_expected < 0 and
 * expected with n_expected < 1 or resolution_bp < 1.
 */
int cgcn_hic_count_dist(cgcn_stream_t stream, long long M, const int32_t *pos1, const int32_t *pos2,
                        const int32_t *window_start, int N, long long min_distance_bp, void *workspace,
                        size_t workspace_bytes, long long *n_survivors);

int cgcn_hic_build_dist(cgcn_stream_t stream, long long M, const int32_t *pos1, const int32_t *pos2, const double *count,
                        const double *norm, long long n_bins, int resolution_bp, const int32_t *window_start, int N,
                        long long K, long long capacity, long long min_distance_bp, const double *expected,
                        long long n_expected, void *workspace, size_t workspace_bytes, int32_t *rowptr_out,
                        int32_t *col_out, int32_t *nnz_out, long long *n_survivors);

int cgcn_hic_count_up_dist(cgcn_stream_t stream, long long M, const int32_t *pos1, const int32_t *pos2,
                           const int32_t *window_start, int N, int resolution_bp, int window_bp, long long n_window_bins,
                           long long min_distance_bp, void *workspace, size_t workspace_bytes, long long *n_survivors);

int cgcn_hic_build_up_dist(cgcn_stream_t stream, long long M, const int32_t *pos1, const int32_t *pos2,
                           const double *count, const double *norm, long long n_bins, int resolution_bp, int window_bp,
                           long long n_window_bins, const int32_t *window_start, int N, long long K, long long capacity,
                           long long min_distance_bp, const double *expected, long long n_expected, void *workspace,
                           size_t workspace_bytes, int32_t *rowptr_out, int32_t *col_out, int32_t *nnz_out,
                           long long *n_survivors);

/*
 * Distance sums: raw_out[d] = sum of count and act_out[d] = sum of count / (nv[b1] * nv[b2]) over the records with
 * |b1 - b2| = d, b = pos / resolution_bp; both fp64 [n_bins], every entry written.  norm fp64 [n_norm] or NULL (act = raw)
 * reads as in cgcn_hic_build: NaN, 0 and a bin outside the vector are +inf, such a record adds 0 to act.  The sums are
 * ordered (a stable sort by distance, fixed tiles of 64 sorted records, one ordered fold of the tile partials): the same
 * bits in every run, exact for integer counts below 2^53, no floating-point atomics.
 * sizes (device uint64 [2]) is written by the call: [0] flags -- 1: a count that is negative or not finite, 2: a negative
 * position, 4: a bin >= n_bins; a flagged record is left out and the caller is expected to refuse the result -- [1]: the
 * largest bin + 1.  n_bins = 0: only `sizes` is computed (raw_out, act_out may be NULL), so that a caller can size n_bins.
 * Enqueue only, no allocation, no sync.  CGCN_ERR_BAD_ARG: a negative size, resolution_bp < 1, a NULL buffer that would be
 * read or written, norm with n_norm < 1; CGCN_ERR_UNSUPPORTED: M >= 2^31 or n_bins >= 2^31 - 1; CGCN_ERR_WORKSPACE:
 * workspace_bytes below cgcn_hicdist_workspace_bytes(M, n_bins), which is 0 for unsupported sizes.
 */
size_t cgcn_hicdist_workspace_bytes(long long M, long long n_bins);

int cgcn_hicdist_sums(cgcn_stream_t stream, long long M, const int32_t *pos1, const int32_t *pos2, const double *count,
                      const double *norm, long long n_norm, int resolution_bp, long long n_bins, void *workspace,
                      size_t workspace_bytes, double *raw_out, double *act_out, unsigned long long *sizes);

/*
 * Hi-C contact text (a Juicer `RAWobserved` dump: data/7create_graph_new.py:71-76 reads it with int() and float()) parsed
 * on the device into pos1 / pos2 / count, the arrays cgcn_hic_count and cgcn_hic_build take (chromegcn_amd/hic.py,
 * DESIGN.md section 4.6).  Additions to ABI 26 like the Hi-C functions above; nothing above changes.
 *
 * THE RULE.  A file is a sequence of lines.  Each line ends with LF or CR LF; the last line may have no terminator (a CR is
 * part of the terminator only in front of an LF).  Record r is the r-th line (0-based); the empty piece behind a final
 * terminator is no line; an empty file has no record.  A line is F1 TAB F2 TAB F3.
 *   FAST (decided and parsed on the device): the line is at most CGCN_TEXT_LINE_MAX bytes without its terminator; F1 and
 *     F2 are one to ten decimal digits with a value below 2^31; F3 is [+-]? digits [. digits]? ([eE] [+-]? digits)?; its
 *     significand digits (integer part, then fraction), without leading zeros and without trailing zeros of the fraction,
 *     are at most 15 and form the integer w < 10^15 < 2^53; e = exponent - (fraction digits that remain in w) has
 *     |e| <= 22.  The value is (double)w * 10^e for e >= 0 and (double)w / 10^-e otherwise, negated behind '-': one
 *     correctly rounded fp64 operation on two exact operands, hence what Python's float() returns, bit for bit.
 *   SLOW: not fast, but float(F3), int(float(F1)) and int(float(F2)) of Python accept the fields and the two positions fit
 *     int32: 16 or more significant digits, |e| > 22, nan / inf counts, 1e3 as a position, blanks around a field, a line
 *     longer than the bound.  The device leaves pos1[r], pos2[r], count[r] of such a line untouched and reports it; the
 *     caller parses exactly those lines on the host and patches them in.
 *   MALFORMED: everything else -- an empty line, a field count other than three, a '#' comment, a field float() rejects.
 * The device decides fast exactly.  Of the other lines it reports as CGCN_TEXT_MALFORMED the ones that are empty or (within
 * the bound) do not hold exactly two TABs, and every remaining one as CGCN_TEXT_SLOW: whether float() accepts those is the
 * host's to say.
 *
 * text: n_bytes bytes, 16-byte aligned.  cgcn_text_count leaves the record count in n_records (device int64 [1]); the caller
 * reads it once, sizes pos1_out / pos2_out int32 [M] and count_out fp64 [M] with it and calls cgcn_text_parse (a smaller M
 * parses the first M records; nothing is overrun).  flags: int64 [flag_capacity][3] = (record, byte offset of its line,
 * kind), appended in any order; flag_totals (device int64 [2]): the number of slow and of malformed lines of the whole
 * text.  When their sum exceeds flag_capacity only flag_capacity entries were written: call again with a larger one.
 * Enqueue only, no allocation, no sync, nothing kept between calls (cgcn_text_parse counts again by itself).
 * CGCN_ERR_BAD_ARG: a negative size, a NULL or misaligned buffer that would be read or written; CGCN_ERR_UNSUPPORTED:
 * M >= 2^31; CGCN_ERR_WORKSPACE: workspace_bytes below cgcn_text_workspace_bytes(n_bytes).
 */
#define CGCN_TEXT_LINE_MAX 64
#define CGCN_TEXT_SLOW 1
#define CGCN_TEXT_MALFORMED 2

size_t cgcn_text_workspace_bytes(long long n_bytes);

int cgcn_text_count(cgcn_stream_t stream, const void *text, long long n_bytes, void *workspace, size_t workspace_bytes,
                    long long *n_records);

int cgcn_text_parse(cgcn_stream_t stream, const void *text, long long n_bytes, long long M, int32_t *pos1_out,
                    int32_t *pos2_out, double *count_out, long long *flags, long long flag_capacity,
                    long long *flag_totals, void *workspace, size_t workspace_bytes);

/*
 * Exact t-SNE of n points into the plane (the class-embedding maps of scripts/visualize.py:148-188, which call scikit-learn's
 * TSNE thirteen times; chromegcn_amd/tsne.py).  Additions to ABI 26 like the functions above; nothing
 * above changes.  The objective is scikit-learn's method='exact' form (sklearn/manifold/_t_sne.py: _joint_probabilities,
 * _kl_divergence at one degree of freedom, _gradient_descent), function by function.
 *
 * Shapes: 2 <= n, n * n < 2^31, d >= 4 and d % 4 == 0; anything else is CGCN_ERR_UNSUPPORTED, decided before any pointer is
 * looked at.  Every n x n matrix (D, C, P) is row-major fp32 with the row pitch ld = (n + 3) & ~3 floats and a 16-byte
 * aligned base; the columns n .. ld - 1 are never read for their value and never written.  X is [n, d] fp32, 16-byte aligned;
 * Y, update, gains and grad are [n, 2] fp32.  eps = 2.220446049250313e-16 throughout.
 * Enqueue only, no allocation, no sync; no atomics and a fixed reduction order in every kernel: the same inputs give the
 * same bits.  One workspace of cgcn_tsne_workspace_bytes(n) bytes (0 for an unsupported n) serves every call; it carries
 * Z and the KL row partials from cgcn_tsne_gradient to the cgcn_tsne_update behind it.
 *
 * cgcn_tsne_sqdist      D[i,j] = sum_k (x_ik - x_jk)^2 in fp32, in the difference form and one order over k: the diagonal is
 *                       exactly 0 and D[i,j] == D[j,i] bit for bit.
 * cgcn_tsne_affinities  the conditional row C[i,:] of _binary_search_perplexity: beta starts at 1, at most 100 steps, entropy
 *                       H = log S + beta (sum_j D_ij e^(-beta D_ij)) / S with S = sum_{j != i} e^(-beta D_ij) (a zero S reads
 *                       1e-8), stop at |H - log perplexity| <= 1e-5; beta doubles (H too large) or halves while the other
 *                       bound is unknown, then moves to the midpoint.  The search is float64 on the fp32 D; perplexity is
 *                       taken as the fp32 it is passed as.  C[i,j] = e^(-beta D_ij) / S as fp32 with the LAST EVALUATED beta,
 *                       C[i,i] = 0; beta[i] (fp64) is that beta.
 * cgcn_tsne_symmetrize  P = max((C + C^T) / sum (C + C^T), eps), the diagonal 0 (scikit-learn keeps the condensed form, which
 *                       has none); the total in float64 in two stages.  P == C (in place) is allowed.
 * cgcn_tsne_gradient    with w_ij = 1 / (1 + |y_i - y_j|^2): Z = sum_{i != j} w_ij (fp32 per row, float64 over rows, left in
 *                       the workspace), then one pass over P: grad[i] = 4 sum_j (e P_ij - max(w_ij / Z, eps)) w_ij (y_i - y_j)
 *                       with e = exaggeration, and when want_kl the row partials of
 *                       KL = sum_ij e P_ij log(max(e P_ij, eps) / max(w_ij / Z, eps)).  P's diagonal must be 0.
 * cgcn_tsne_update      _gradient_descent's body: gains += 0.2 where update * grad < 0, gains *= 0.8 elsewhere, floor 0.01;
 *                       grad *= gains; update = momentum update - learning_rate grad; Y += update.  record (fp64 [4], device):
 *                       {KL (NaN unless have_kl; the gradient call before it must have had want_kl), |gains * grad|_2 -- the
 *                       norm _gradient_descent tests --, Z, 0}.  grad itself is left as it was.
 * CGCN_ERR_BAD_ARG: a NULL or misaligned buffer, a perplexity that is not positive; CGCN_ERR_WORKSPACE: workspace_bytes below
 * cgcn_tsne_workspace_bytes(n).
 */
size_t cgcn_tsne_workspace_bytes(int n);

int cgcn_tsne_sqdist(cgcn_stream_t stream, int n, int d, int ld, const float *X, float *D);

int cgcn_tsne_affinities(cgcn_stream_t stream, int n, int ld, const float *D, float perplexity, float *C, double *beta);

int cgcn_tsne_symmetrize(cgcn_stream_t stream, int n, int ld, const float *C, float *P, void *workspace,
                         size_t workspace_bytes);

int cgcn_tsne_gradient(cgcn_stream_t stream, int n, int ld, const float *P, const float *Y, float exaggeration, float *grad,
                       int want_kl, void *workspace, size_t workspace_bytes);

int cgcn_tsne_update(cgcn_stream_t stream, int n, float *Y, float *update, float *gains, const float *grad, float momentum,
                     float learning_rate, int have_kl, double *record, void *workspace, size_t workspace_bytes);

/*
 * ROC and precision-recall curves of every label (utils/evals.py:28-84 -> utils/metrics.py:255-303: one scikit-learn
 * roc_curve / precision_recall_curve call per label; chromegcn_amd/curves.py).  These four functions
 * are additions to ABI 26: CGCN_ABI_VERSION stays 26, nothing above changes.
 * Scores are probabilities (non-negative, as for cgcn_multilabel_metrics_nonneg, whose pack and segmented sort run
 * here): a negative score or a NaN sets bad[0] and leaves every output unspecified.  1 <= n, n * C < 2^31, else
 * CGCN_ERR_UNSUPPORTED.  A curve point is the last element of each run of equal scores in a label's descending list
 * (sklearn's _binary_clf_curve): tps = positives down to it, fps = negatives down to it, threshold = that score.
 *
 * Two calls, because only the device knows how many points there are (as cgcn_graph_count / cgcn_graph_fill):
 * cgcn_curves_count    sorts, marks the points and writes offsets (int64 [C + 1], device): label c's points are
 *                      [offsets[c], offsets[c + 1]) of the flat outputs, offsets[C] is their length.
 *                      kind CGCN_CURVE_ROC: every label starts with the origin (0, 0, +inf), as roc_curve prepends it; with
 *                      drop_intermediate != 0 and more than two points, point k stays iff it is the first, the last, or the
 *                      second difference of fps or of tps at k is non-zero (roc_curve's rule, applied before the origin
 *                      is prepended).  kind CGCN_CURVE_PR: the points only; drop_intermediate must be 0.
 * cgcn_curves_fill     writes tps, fps (int32) and thresholds (fp32: the score's own bits, -0 as +0) in descending-score
 *                      order per label, from the workspace the count call left (same n, C, workspace, nothing else run on
 *                      it in between).  capacity: elements each output holds; nothing is written at or past it.
 * cgcn_curves_cutoff   from a filled ROC curve: cutoffs[c] (fp32 [C]) = threshold of the first point that minimises
 *                      |tps / P - (1 - fps / N)| in float64, P / N the label's positives / negatives (Find_Optimal_Cutoff,
 *                      utils/metrics.py:224-235); NaN without a positive or without a negative.  No workspace.
 * Enqueue only: no allocation, no sync, nothing kept between calls but the workspace contents; integer counts throughout,
 * so the same inputs give the same bits.  cgcn_curves_workspace_bytes is 0 for an unsupported size.
 */
#define CGCN_CURVE_ROC 0
#define CGCN_CURVE_PR 1

size_t cgcn_curves_workspace_bytes(long long n, int C);

int cgcn_curves_count(cgcn_stream_t stream, long long n, int C, const float *probs, const float *targets, int kind,
                      int drop_intermediate, long long *offsets, int32_t *bad, void *workspace, size_t workspace_bytes);

int cgcn_curves_fill(cgcn_stream_t stream, long long n, int C, const long long *offsets, long long capacity, int32_t *tps,
                     int32_t *fps, float *thresholds, void *workspace, size_t workspace_bytes);

int cgcn_curves_cutoff(cgcn_stream_t stream, int C, const long long *offsets, const int32_t *tps, const int32_t *fps,
                       const float *thresholds, float *cutoffs);

/*
 * Thresholded multi-label counts (utils/metrics.py:29-109 behind utils/evals.py:94-100's -br_threshold: subset accuracy,
 * Hamming loss, example-based / micro / macro F1; chromegcn_amd/thresholds.py).  These three
 * functions are additions to ABI 26: CGCN_ABI_VERSION stays 26, nothing above changes.
 * With Y[i][c] = targets[i][c] > 0.5f and P[t][i][c] = probs[i][c] >= thresholds[t][c] in float32 (a NaN probability is
 * never predicted; thresholds [T][C] may be +-inf), one stream over probs and targets ([n][C] row-major) writes, as int64:
 *   pos[c]        rows with Y                                  [C]
 *   tp[t][c]      rows with P and Y                            [T][C]
 *   pp[t][c]      rows with P (fp = pp - tp, fn = pos - tp)    [T][C]
 *   exact[t]      rows whose C decisions equal their C targets [T]
 *   rows[t][k]    rows with |P_i| + |Y_i| = k, k = 0 .. 2C     [T][2C + 1]
 *   tpsum[t][k]   sum of |P_i and Y_i| over those rows         [T][2C + 1]
 * (sum_i 2 tp_i / (|P_i| + |Y_i|) = sum_k (2 / k) tpsum[k]: the example-based F1 without a floating-point sum over rows.)
 * Every element of every output is written; callers do not clear them.  1 <= n < 2^47, 1 <= C <= 1024, 1 <= T <= 64,
 * else CGCN_ERR_UNSUPPORTED and cgcn_threshold_workspace_bytes is 0.  Enqueue only: no allocation, no sync; integer sums, so
 * the same inputs give the same bits.  The workspace is reserved: it must be given at the queried size and is not written.
 * cgcn_debug_threshold_route: the number of passes over the rows the call makes (thresholds are taken in groups whose row
 * histograms fit the LDS: 1 = one pass; more = the slow route of large C * T), or CGCN_ERR_UNSUPPORTED.  Host logic only.
 */
size_t cgcn_threshold_workspace_bytes(long long n, int C, int T);

int cgcn_debug_threshold_route(long long n, int C, int T);

int cgcn_threshold_counts(cgcn_stream_t stream, long long n, int C, int T, const float *probs, const float *targets,
                          const float *thresholds, long long *pos, long long *tp, long long *pp, long long *exact,
                          long long *rows, long long *tpsum, void *workspace, size_t workspace_bytes);

/*
 * KR / VC / SQRTVC normalisation vectors of a Hi-C contact matrix from the contact records (chromegcn_amd/hicnorm.py,
 * DESIGN.md section 4.10).  These seven functions are additions to ABI 26: CGCN_ABI_VERSION stays 26, nothing above changes.
 * Enqueue only: no allocation, no synchronisation, caller-owned workspace and state, no floating-point atomics -- the same
 * inputs give the same bits in every run.
 *
 * The matrix A (n_bins x n_bins, symmetric, fp64): a record (pos1, pos2, c) with i = pos1 / resolution_bp, j = pos2 /
 * resolution_bp adds c to A[i][i] when i == j and to A[i][j] and A[j][i] otherwise; the records of one entry are added in
 * record order.  cgcn_hicnorm_count writes sizes[0] = the number of stored entries, sizes[1] = flags (1: a count that is
 * negative or not finite, 2: a negative position, 4: a bin >= n_bins when n_bins > 0; such records are left out),
 * sizes[2] = the largest bin + 1; sizes holds four int64.  n_bins = 0 there: not known yet.  cgcn_hicnorm_fill writes the
 * CSR (rowptr [n_bins + 1], col and val [capacity], columns ascending, duplicates merged), vc[i] = the sum of row i (in the
 * order of cgcn_hicnorm_spmv's default route), row_nnz[i] = its entries > 0, and sizes again; capacity >= sizes[0], or the
 * matrix is cut off behind `capacity` entries (no row pointer exceeds it; sizes[0] tells).  M < 2^31 - 1, n_bins < 2^31 - 1, capacity < 2^31 - 1,
 * and for cgcn_hicnorm_fill 2 bits(n_bins) + bits(M) + 1 <= 64 (the sort key holds row, column and record index: 250 000 bins
 * with 1.3 * 10^8 records fit, 2^20 bins with more than 2^23 records do not), else CGCN_ERR_UNSUPPORTED and
 * cgcn_hicnorm_workspace_bytes(M, n_bins) is 0.
 *
 * cgcn_hicnorm_spmv: y = mask o (A (mask o x o p)), o the elementwise product; mask (0 / 1 as fp64), x and p may each be
 * NULL (all ones).  A row with more than long_row_nnz entries is summed by a whole workgroup, any other by 16 lanes;
 * long_row_nnz < 0: the default (512); 0: every non-empty row takes the workgroup route.  The two routes add in different
 * orders, each in a fixed one.
 *
 * Knight-Ruiz balancing (Knight & Ruiz 2013, inner-outer Newton with CG; the listing is in chromegcn_amd/hicnorm.py) is
 * driven by the host, one bounded step per call.  The state (cgcn_hicnorm_kr_state_bytes(n) bytes, 8-byte aligned) is
 * CGCN_HICNORM_HDR fp64 (the record, then reduction partials) followed by eleven vectors of stride (n + 31) & ~31 fp64 in
 * the order CGCN_HICNORM_VEC_*: mask, x, v, p, w, y[2], rk[2], Z[2]; `parity` names the current copy of y, rk and Z.
 * Record, fp64: [0] rho1, [1] rho2, [2] p.w, [3] min ynew, [4] max ynew, [5] gamma of the lower bound, [6] gamma of the
 * upper bound, [7] rho1 after the step, [8] rout, [9] alpha, [10] kept rows, [11] non-empty rows.  Steps (w holds a product
 * of cgcn_hicnorm_spmv where one is named):
 *   CGCN_HICNORM_OP_MASK   mask = vc > 0 and row_nnz >= flag; x = y = 1; [10], [11]
 *   CGCN_HICNORM_OP_RES    w = product(x, p = y when flag, else p = NULL); x *= y (flag); v = x o w; rk = mask o (1 - v);
 *                          y = 1; [0] = [8] = rk.rk
 *   CGCN_HICNORM_OP_FIRST  Z = rk / v; p = Z; [0] = rk.Z
 *   CGCN_HICNORM_OP_DIR    p = Z + ([7] / [0]) p   (after an accepted step, whose copy `parity` now names)
 *   CGCN_HICNORM_OP_W      w = product(x, p); w = x o w + v o p; flag: [1] = [0], [0] = [7] first; [2] = p.w; [9] = [0] / [2]
 *   CGCN_HICNORM_OP_Y      the other copy: ynew = y + [9] p, rk - [9] w, Z = that / v; [3] .. [7]
 *   CGCN_HICNORM_OP_CLIP   y += gamma ([9] p), gamma = [5] (flag 0) or [6] (flag 1)
 * cgcn_hicnorm_vector: kind 0: out = vc, 1: sqrt(vc), both NaN where vc is not > 0; 2: 1 / x on the kept rows of `state`,
 * NaN elsewhere.
 * CGCN_ERR_BAD_ARG: a negative size, resolution_bp < 1, a NULL buffer that would be read or written, an unknown op, kind or
 * parity; CGCN_ERR_WORKSPACE: workspace_bytes / state_bytes below the queried size.
 */
#define CGCN_HICNORM_REC 32
#define CGCN_HICNORM_HDR (CGCN_HICNORM_REC + 6 * 1024)
#define CGCN_HICNORM_OP_MASK 0
#define CGCN_HICNORM_OP_RES 1
#define CGCN_HICNORM_OP_FIRST 2
#define CGCN_HICNORM_OP_DIR 3
#define CGCN_HICNORM_OP_W 4
#define CGCN_HICNORM_OP_Y 5
#define CGCN_HICNORM_OP_CLIP 6
#define CGCN_HICNORM_VEC_MASK 0
#define CGCN_HICNORM_VEC_X 1
#define CGCN_HICNORM_VEC_V 2
#define CGCN_HICNORM_VEC_P 3
#define CGCN_HICNORM_VEC_W 4
#define CGCN_HICNORM_VEC_Y 5
#define CGCN_HICNORM_VEC_RK 7
#define CGCN_HICNORM_VEC_Z 9

size_t cgcn_hicnorm_workspace_bytes(long long M, long long n_bins);

int cgcn_hicnorm_count(cgcn_stream_t stream, long long M, const int32_t *pos1, const int32_t *pos2, const double *count,
                       int resolution_bp, long long n_bins, void *workspace, size_t workspace_bytes, long long *sizes);

int cgcn_hicnorm_fill(cgcn_stream_t stream, long long M, const int32_t *pos1, const int32_t *pos2, const double *count,
                      int resolution_bp, long long n_bins, long long capacity, void *workspace, size_t workspace_bytes,
                      int32_t *rowptr, int32_t *col, double *val, double *vc, int32_t *row_nnz, long long *sizes);

int cgcn_hicnorm_spmv(cgcn_stream_t stream, int n, const int32_t *rowptr, const int32_t *col, const double *val,
                      const double *mask, const double *x, const double *p, double *y, int long_row_nnz);

size_t cgcn_hicnorm_kr_state_bytes(int n);

int cgcn_hicnorm_kr_step(cgcn_stream_t stream, int n, int op, int flag, int parity, const double *vc, const int32_t *row_nnz,
                         void *state, size_t state_bytes);

int cgcn_hicnorm_vector(cgcn_stream_t stream, int n, int kind, const double *vc, const void *state, double *out);

/*
 * Read-pair text (a HiC-Pro `allValidPairs` file: one line per read pair, as data/eqtl_data/HiChIP.py:8-24 reads it) turned on
 * the device into binned pairs and into contact records, the arrays cgcn_hic_count, cgcn_hic_build and cgcn_hicnorm_* take
 * (chromegcn_amd/pairs.py).  Additions to ABI 26 like the functions above; nothing above changes.
 *
 * THE RULE.
 * Lines.  A line ends with LF or CR LF; the last line may end with nothing.  An empty line is skipped, as csv.DictReader
 *   skips it.  A line has at least six TAB-separated fields (read name, chr1, pos1, strand1, chr2, pos2, ...); fields 2, 3, 5
 *   and 6 are used and the rest are ignored.  Line numbers count every line, empty ones included, from 0.
 * Parameters.  chroms: 1 to CGCN_PAIRS_MAX_CHROMS names of 1 to CGCN_PAIRS_NAME_MAX bytes each.  resolution_bp >= 8.
 *   binning: CGCN_PAIRS_NEAREST is the reference's round(int(pos), -3) generalised -- with q, r = divmod(pos, resolution_bp):
 *   q when 2 r < res, q + 1 when 2 r > res, the even one of the two on a tie; times resolution_bp.  CGCN_PAIRS_FLOOR is
 *   pos - pos % resolution_bp, the binning of Juicer's dumps and of data/7create_graph_old.py:89.  min_diff: a pair is kept iff
 *   |p2 - p1| > min_diff on the binned positions (the reference: 10).
 * Fate of a pair.  Field 2 != field 5 (byte for byte): dropped, counted as inter_chrom, its positions are not looked at.
 *   Otherwise both positions are read and binned; then a name that is not in chroms: dropped, other_chrom; a pair that fails
 *   min_diff: dropped, too_close; else kept.
 * Classes of line.
 *   FAST (decided and parsed on the device): at most CGCN_PAIRS_LINE_MAX bytes without its terminator, six or more fields,
 *     fields 3 and 6 one to ten plain digits with a value below 2^31, fields 2 and 5 of 1 to CGCN_PAIRS_NAME_MAX bytes, no `"`
 *     byte and no CR other than the one of a CR LF.
 *   SLOW: not fast, but the reference's statements accept it: blanks, `+` or `_` inside int(), a longer line, a longer name.
 *     The device reports it; the caller runs the host rule on exactly those lines and merges their pairs in at their input
 *     positions.
 *   MALFORMED: everything else -- fewer than six fields, a position int() refuses (on a line whose two names are equal), a
 *     negative position, a binned position >= 2^31, a `"` byte, a lone CR.
 *   The device decides fast exactly.  Of the other lines it reports as CGCN_PAIRS_MALFORMED the ones that (within the bound)
 *   hold fewer than five TABs, a `"`, a lone CR or a binned position >= 2^31, and every remaining one as CGCN_PAIRS_SLOW:
 *   what the reference's statements make of a reported line is the host's to say.
 *
 * STAGE A, binned pairs: cgcn_pairs_parse takes one chunk of whole lines (text: n_bytes bytes, 16-byte aligned, the bytes
 * byte_base .. of the file) and appends the keys of its kept pairs, in input order, to keys (device uint64 [key_capacity])
 * behind the keys of the earlier chunks.  A key is  chromosome index << 57 | lo << 29 | hi << 1 | swapped  with
 * lo = min(p1, p2) / res, hi = max(p1, p2) / res (28 bits each: binned positions are below 2^31 and res >= 8) and
 * swapped = 1 when p1 > p2; bit 63 is 0.  names: device bytes [n_chroms][16], 8-byte aligned -- a name's bytes, zeros, and its
 * length in byte 15.  totals (device int64 [8], the CGCN_PAIRS_T_* words; the caller zeroes it before the first chunk): the
 * running totals; the call starts its line numbers at totals[CGCN_PAIRS_T_LINES] and its keys at totals[CGCN_PAIRS_T_KEPT]
 * and adds the chunk's totals, which it also leaves in chunk_totals (device int64 [8]).  A key whose index is key_capacity or
 * more is not written (the totals still count it).  flags: int64 [flag_capacity][4] = (line, byte offset of the line in the
 * file, kind, number of keys in front of the line once this call's keys are in place), appended in any order from entry 0 in
 * every call; when the chunk's slow + malformed lines exceed flag_capacity only flag_capacity entries were written: restore
 * totals and call again with a larger one.
 *
 * STAGE B, contact records (this project's definition, not the reference's, which stops at the binned pairs and never
 * aggregates them: it is the one Juicer's `dump observed` would give for the same pairs): cgcn_pairs_reduce sorts n_keys keys
 * and writes, per chromosome in table order, one record for every distinct unordered bin pair -- pos1 = lo * res,
 * pos2 = hi * res (int32), count = the number of kept pairs (fp64) -- sorted by (pos1, pos2).  pos1_out / pos2_out / count_out
 * hold n_keys entries; n_records (device int64 [1]) receives the record count and chrom_offsets (device int64 [n_chroms + 1])
 * the first record of every chromosome.  keys is left as it is.
 *
 * Enqueue only, no allocation, no sync, nothing kept between calls except what the caller passes back in.  Integer arithmetic
 * throughout; the one conversion is count's.  CGCN_ERR_BAD_ARG: a negative size, an unknown binning, a NULL or misaligned
 * buffer; CGCN_ERR_UNSUPPORTED: n_chroms outside 1 .. CGCN_PAIRS_MAX_CHROMS or resolution_bp < 8 (the key has no room for
 * them), n_keys >= 2^31 - 1; CGCN_ERR_WORKSPACE: workspace_bytes below cgcn_pairs_parse_workspace_bytes(n_bytes) /
 * cgcn_pairs_reduce_workspace_bytes(n_keys).
 */
#define CGCN_PAIRS_LINE_MAX 256
#define CGCN_PAIRS_NAME_MAX 15
#define CGCN_PAIRS_MAX_CHROMS 64
#define CGCN_PAIRS_SLOW 1
#define CGCN_PAIRS_MALFORMED 2
#define CGCN_PAIRS_NEAREST 0
#define CGCN_PAIRS_FLOOR 1
#define CGCN_PAIRS_T_LINES 0
#define CGCN_PAIRS_T_EMPTY 1
#define CGCN_PAIRS_T_KEPT 2
#define CGCN_PAIRS_T_INTER_CHROM 3
#define CGCN_PAIRS_T_OTHER_CHROM 4
#define CGCN_PAIRS_T_TOO_CLOSE 5
#define CGCN_PAIRS_T_SLOW 6
#define CGCN_PAIRS_T_MALFORMED 7

size_t cgcn_pairs_parse_workspace_bytes(long long n_bytes);

int cgcn_pairs_parse(cgcn_stream_t stream, const void *text, long long n_bytes, long long byte_base, const void *names,
                     int n_chroms, int resolution_bp, int binning, long long min_diff, unsigned long long *keys,
                     long long key_capacity, long long *flags, long long flag_capacity, long long *totals,
                     long long *chunk_totals, void *workspace, size_t workspace_bytes);

size_t cgcn_pairs_reduce_workspace_bytes(long long n_keys);

int cgcn_pairs_reduce(cgcn_stream_t stream, long long n_keys, const unsigned long long *keys, int n_chroms, int resolution_bp,
                      int32_t *pos1_out, int32_t *pos2_out, double *count_out, long long *chrom_offsets,
                      long long *n_records, void *workspace, size_t workspace_bytes);

/*
 * Label and Hi-C neighbourhood statistics (chromegcn_amd/labelstats.py): what
 * scripts/analyze_results.py:226-266 (get_label_weights) and utils/util_methods.py:24-74 (summarize_data) count, as exact
 * integers, from tensors that are already on the device.  Additions to ABI 26 like the functions above: CGCN_ABI_VERSION stays
 * 26, nothing above changes.
 *
 * targets: float32 [n, C], 1 <= C <= CGCN_LABELSTATS_MAX_C.  Window u is positive for label c iff targets[u, c] != 0 (the
 * ablation's rule; NaN is positive); P_c is the set of such windows.
 *
 * cgcn_labelstats_windows packs the label bits into `workspace` (uint64 [n][W], W = (C + 63) / 64, bit l of word w = label
 * 64 w + l; at least cgcn_labelstats_workspace_bytes(n, C) bytes, 0 = unsupported) and writes, all int64:
 *   label_count  [C]       |P_c|
 *   labels_hist  [C + 1]   windows with exactly k positive labels
 *   cooccurrence [C, C]    |P_a and P_b|
 * cgcn_labelstats_graph takes one chromosome's CSR (n rows, int32, nnz entries; val NULL = every value is 1) and the packed
 * bits the window call left in its workspace (label_bits, label_bits_bytes of them).  A neighbour entry is a stored entry
 * (u, v) with u != v and, where val is given, val > 0; deg[u] is their number in row u.  A column outside [0, n) is never
 * dereferenced and not counted.  It writes, all int64:
 *   degree_sum    [C]      sum of deg[u] over P_c
 *   contact_pairs [C, C]   neighbour entries (u, v) with u in P_a and v in P_b (directed entries)
 *   n_entries     [1]      sum of deg[u] over every row
 * accumulate: 0 zeroes the outputs first, 1 adds into them (the statistics of several chromosomes add element-wise).
 *
 * Enqueue only, no allocation, no sync.  Integer arithmetic only: results are exact and identical from call to call.
 * CGCN_ERR_UNSUPPORTED (decided before any pointer is looked at): C < 1, C > CGCN_LABELSTATS_MAX_C, nnz >= 2^31;
 * CGCN_ERR_BAD_ARG: a negative size, a NULL buffer that would be read or written; CGCN_ERR_WORKSPACE: workspace_bytes /
 * label_bits_bytes below the queried size.  n = 0 launches nothing and still zeroes the outputs when accumulate = 0.
 */
#define CGCN_LABELSTATS_MAX_C 256

size_t cgcn_labelstats_workspace_bytes(int n, int C);

int cgcn_labelstats_windows(cgcn_stream_t stream, int n, int C, const float *targets, void *workspace, size_t workspace_bytes,
                            long long *label_count, long long *labels_hist, long long *cooccurrence, int accumulate);

int cgcn_labelstats_graph(cgcn_stream_t stream, int n, int C, long long nnz, const int32_t *rowptr, const int32_t *col,
                          const float *val, const void *label_bits, size_t label_bits_bytes, long long *degree_sum,
                          long long *contact_pairs, long long *n_entries, int accumulate);

/*
 * Window effects through the Hi-C graph (chromegcn_amd/effects.py).  Additions to ABI 26 like the
 * functions above: CGCN_ABI_VERSION stays 26, nothing above changes.
 *
 * Variant m replaces the input row of window u = windows[m] by alt[m] ([n_var][S][d]) in both strands of an eval forward.
 * Its INSTANCES are the rows whose layer-1 value changes: instance 0 is u itself; after it comes every v != u with a stored
 * A[v, u], in the stored order of row u of the transpose (rowptr_t, col_t, val_t; rows sorted and duplicate-free).  A self
 * loop does not repeat u, and a graph without a stored diagonal still has instance 0.
 *
 * cgcn_effects_plan: counts [n_var] (instances of every variant, >= 1) and diag_pos [n_var] (position of the stored (u, u)
 * inside the transposed row, -1 without one).  The caller forms offsets int64 [n_var + 1] = exclusive prefix sums.
 *
 * The instance tables are [S][rows][d] fp32, i.e. feature tables with n = rows.  A call covers the n_var variants whose
 * windows, alt, offsets and diag_pos entries the pointers start at (a batch: offsets[0] need not be 0).
 *   own = 0: table row i is the instance offsets[0] + i of the batch; n_inst = offsets[n_var] - offsets[0].
 *   own = 1: table row i is instance 0 of variant i; n_inst = n_var.
 *
 * cgcn_effects_rows1, layer 1, from the unperturbed layer input X0 [S, n, d] and its saved aggregation H1 [S, n, d]
 * (cgcn_layer_fwd's H): for the instance with window v
 *   H_inst = H1[s, v] + (row_scale[v] * val_t[v, u]) * (alt[m, s] - X0[s, u])   one fused multiply-add per element
 *            (val_t NULL: 1; row_scale NULL: 1; instance 0 without a stored diagonal: H1[s, u] unchanged),
 *   X_inst = alt[m, s] for instance 0, X0[s, v] otherwise (the layer's residual input),
 *   rows[i] = v (rows may be NULL).
 * cgcn_layer_fwd with H_in = H_inst, X = X_inst and n = n_inst then gives the instances' layer-1 output.
 *
 * cgcn_effects_rows2, layer 2, from the unperturbed X1, H2 [S, n, d] and the instances' layer-1 output X1_inst
 * [S][n_inst][d] (always the own = 0 table of the same batch): for every read-out row (own as above; n_out = n_var or
 * n_inst rows)
 *   H_out = H2[s, v] + row_scale[v] * sum_w val[v, w] * (X1_inst[s, instance of w] - X1[s, w])
 * over the stored entries w of row v of (rowptr, col, val) that are instances of the same variant (w = u is instance 0; else
 * w is looked up in the transposed row of u), added in ascending w; X_res = X1_inst[s, the row's own instance] (required
 * when own = 1, may be NULL when own = 0: X1_inst is then the residual table itself).
 *
 * cgcn_effects_workspace_bytes: what chromegcn_amd/effects.py carves for a batch of n_inst instances, or 0 when unsupported:
 *   [H_inst][X_inst][X1_inst][X2_inst: layers == 2] of n_inst * S * d fp32 each, [gate: n_inst * S fp32],
 * each part starting at a 256-byte boundary.
 *
 * Enqueue only: no allocation, no synchronisation, caller-owned buffers, legal under graph capture.  No atomics: results are
 * bit-identical from call to call.  S must be 2 and d 128 or 256, else CGCN_ERR_UNSUPPORTED (layers outside {1, 2}: 0 bytes);
 * NULL required buffers, negative sizes, a table that is not 16-byte aligned: CGCN_ERR_BAD_ARG, before any launch.
 */
size_t cgcn_effects_workspace_bytes(int n_inst, int S, int d, int layers);

int cgcn_effects_plan(cgcn_stream_t stream, int n, const int32_t *rowptr_t, const int32_t *col_t, int n_var,
                      const int32_t *windows, int32_t *counts, int32_t *diag_pos);

int cgcn_effects_rows1(cgcn_stream_t stream, int n, int S, int d, const int32_t *rowptr_t, const int32_t *col_t,
                       const float *val_t, const float *row_scale, const float *X0, const float *H1, const int32_t *windows,
                       const float *alt, const long long *offsets, const int32_t *diag_pos, int n_var, int own, int n_inst,
                       float *H_inst, float *X_inst, int32_t *rows);

int cgcn_effects_rows2(cgcn_stream_t stream, int n, int S, int d, const int32_t *rowptr, const int32_t *col, const float *val,
                       const float *row_scale, const int32_t *rowptr_t, const int32_t *col_t, const float *X1, const float *H2,
                       const int32_t *windows, const long long *offsets, const int32_t *diag_pos, int n_var, int own, int n_inst,
                       const float *X1_inst, float *H_out, float *X_res);

/*
 * Random contact graphs that keep the distance histogram or the degrees of a Hi-C graph (chromegcn_amd/nullgraph.py, whose
 * docstring is the rule).  Additions to ABI 26 like the functions above: CGCN_ABI_VERSION stays 26,
 * nothing above changes.
 *
 * Input: the CSR (rowptr [n + 1], col) of a graph on n windows, nnz = the number of entries col holds for it (rowptr is
 * clamped to it); only the entries (i, j) with j > i count, in storage order.  model: CGCN_NULL_DISTANCE (placement with
 * `rounds` rounds of retries, per-distance classes, complemented where more than half full), CGCN_NULL_DEGREE (erased
 * configuration model; rounds is ignored but must be >= 1), CGCN_NULL_UNIFORM (placement of m pairs).  seed: 64 bits, both
 * halves matter.
 *
 * Output: rowptr_out int32 [n + 1] and col_out int32 [capacity] -- the canonical symmetric CSR without a diagonal, columns
 * ascending; col_out behind the last entry is zero.  capacity >= 1 is the room of col_out: 2 nnz is enough for DEGREE and
 * UNIFORM, 4 nnz for DISTANCE (an unplaced hole of a complemented class adds an edge).  Nothing is written behind it: entries
 * that do not fit are dropped and CGCN_NULL_FLAG_OVERRUN is set.
 * sizes int64 [10], on the device: [0] entries written (= rowptr_out[n]), [1] edges in (m), [2] edges out, [3] tokens
 * (DISTANCE: holes or edges per class; UNIFORM: m; DEGREE: the 2 m stubs), [4] unplaced tokens, [5] complemented classes,
 * [6] loops, [7] repeats, [8] the number of rounds that had losers, [9] CGCN_NULL_FLAG_* bits: OVERRUN; UNSUPPORTED (UNIFORM
 * with m > 0 and n < 2 or 4 m > n (n - 1): the graph is empty); BAD_INDEX (a column outside [0, n) was skipped).
 *
 * Enqueue only: no allocation, no synchronisation, nothing kept between calls; the result is a pure function of the input
 * and the seed (integer atomics and sorts only).  CGCN_ERR_BAD_ARG: a negative size, capacity or rounds < 1, an unknown
 * model, a NULL buffer that would be read or written; CGCN_ERR_UNSUPPORTED: nnz >= 2^30, capacity >= 2^31, or a key of
 * (window, window, token) that does not fit 63 bits (cgcn_null_graph_workspace_bytes is then 0); CGCN_ERR_WORKSPACE:
 * workspace_bytes below cgcn_null_graph_workspace_bytes(n, nnz, capacity, model).
 */
#define CGCN_NULL_DISTANCE 0
#define CGCN_NULL_DEGREE 1
#define CGCN_NULL_UNIFORM 2
#define CGCN_NULL_FLAG_OVERRUN 1
#define CGCN_NULL_FLAG_UNSUPPORTED 2
#define CGCN_NULL_FLAG_BAD_INDEX 4

size_t cgcn_null_graph_workspace_bytes(int n, long long nnz, long long capacity, int model);

int cgcn_null_graph(cgcn_stream_t stream, int n, long long nnz, const int32_t *rowptr, const int32_t *col, int model,
                    long long seed, int rounds, long long capacity, int32_t *rowptr_out, int32_t *col_out, long long *sizes,
                    void *workspace, size_t workspace_bytes);

/*
 * Weighted ranking sums of every label for many integer weight vectors from one sort: block-bootstrap confidence intervals
 * (chromegcn_amd/bootstrap.py, whose docstring is the rule).  Additions to ABI 26 like the functions
 * above: CGCN_ABI_VERSION stays 26, nothing above changes.
 *
 * Shapes: 1 <= n < 2^23 windows (so that a replicate's total weight, at most 255 n, stays below 2^31), C >= 1 labels with
 * n C <= 2^31 and a key [label | score | target | window] of at most 64 bits (C <= 1024 with n <= 2^21 fits); anything else
 * is CGCN_ERR_UNSUPPORTED and cgcn_bootstrap_workspace_bytes is 0.  R replicates form ceil(R / 64) groups of 64.
 *
 * cgcn_bootstrap_workspace_bytes(n, C, R): what cgcn_bootstrap_sort (n, C) and cgcn_bootstrap_weights (n, R) need, the larger
 * of the two; R = 0 asks for the sort alone.
 * cgcn_bootstrap_sort: probs, targets float [n, C] (a target is positive iff > 0.5; -0 is folded onto +0) -> order uint32
 * [C n], label c's windows by descending score in [c n, (c + 1) n): window index | target << 30 | run end << 31, where a run
 * end is the last element of a group of equal scores.  A NaN score ORs 1 into bad[0] (int32, zeroed by the caller).
 * cgcn_bootstrap_weights: the circular block bootstrap of replicates rep0 .. rep0 + R - 1 (R <= 65535) over the strata
 * [offsets[s], offsets[s + 1]) (int32 [n_strata + 1] on the device, ascending, within [0, n]; empty strata are skipped) with
 * block length `block`; draws = the number of draws of one replicate, sum over the strata of ceil(n_s / min(block, n_s)).
 * tile: bytes [ceil(R / 64)][n][64], the weight of window i in replicate r at ((r / 64) n + i) 64 + r % 64; lanes behind R
 * hold 0.  cgcn_bootstrap_weights_in: the same tile from explicit weights int32 [R, n].
 * flags[0] (int32, zeroed by the caller) collects CGCN_BOOT_FLAG_* bits: WEIGHT (a weight above 255: the byte stored is its
 * low byte and the sums are to be discarded), NEGATIVE (stored as 0), STRATA (offsets outside the rule above).
 * cgcn_bootstrap_sums: out, 6 R C words of 8 bytes: int64 A, P, TOT, F and float64 S_ap, S_pr, each [R, C].
 * fdr_cutoff: a HOST pointer to one float64 in (0, 1), read during the call (CGCN_ERR_BAD_ARG outside the interval).
 *
 * Enqueue only: no allocation, no synchronisation, nothing kept between calls; integer atomics, one sort and sums in a fixed
 * order, so every output is the same bits from run to run.  CGCN_ERR_BAD_ARG: a negative size, R < 1 (sums, weights),
 * block < 1, a NULL buffer; CGCN_ERR_WORKSPACE: workspace_bytes below cgcn_bootstrap_workspace_bytes.
 */
#define CGCN_BOOT_FLAG_WEIGHT 1
#define CGCN_BOOT_FLAG_NEGATIVE 2
#define CGCN_BOOT_FLAG_STRATA 4

size_t cgcn_bootstrap_workspace_bytes(long long n, int C, int R);

int cgcn_bootstrap_sort(cgcn_stream_t stream, long long n, int C, const float *probs, const float *targets, uint32_t *order,
                        int32_t *bad, void *workspace, size_t workspace_bytes);

int cgcn_bootstrap_weights(cgcn_stream_t stream, long long n, long long rep0, int R, int n_strata, const int32_t *offsets,
                           int block, long long draws, long long seed, unsigned char *tile, int32_t *flags, void *workspace,
                           size_t workspace_bytes);

int cgcn_bootstrap_weights_in(cgcn_stream_t stream, long long n, int R, const int32_t *weights, unsigned char *tile,
                              int32_t *flags);

int cgcn_bootstrap_sums(cgcn_stream_t stream, long long n, int C, int R, const uint32_t *order, const unsigned char *tile,
                        const double *fdr_cutoff, long long *out);

/*
 * Diamond sums of a contact matrix, the input of the insulation score (chromegcn_amd/insulation.py, whose docstring is the
 * rule).  An addition to ABI 26 like the functions above: CGCN_ABI_VERSION stays 26, nothing above
 * changes.
 *
 * The matrix is what cgcn_hicnorm_fill writes: n bins, rowptr int32 [n + 1], col int32 and val fp64 [rowptr[n]], symmetric, the
 * columns of a row ascending.  For window k (windows: a HOST array int32 [n_windows], read during the call, 1 <= n_windows <=
 * 8, every window >= 1, strictly ascending) and bin i,
 *   out[k n + i] = sum over a in [max(i - w_k, 0), i - 1], b in [i, min(i + w_k, n) - 1] of val[a, b] / (nv[a] * nv[b]),
 * one fp64 multiplication and one fp64 division per term; norm fp64 [n_norm] or NULL (the terms are val itself) reads as in
 * cgcn_hic_build: NaN, 0 and a bin outside the vector are +inf, such a term adds 0.  out fp64 [n_windows][n], every entry
 * written; out[k n] = 0 and the diagonal never takes part.  One wavefront per bin adds its terms in a fixed order: the same
 * bits in every run, exact for integer counts below 2^53, no floating-point atomics.
 * Enqueue only: no workspace, no allocation, no synchronisation.  CGCN_ERR_BAD_ARG: a NULL pointer that would be read or
 * written, n < 0, n_norm < 0, norm with n_norm < 1, n_windows < 1, a window < 1 or not above the one before it;
 * CGCN_ERR_UNSUPPORTED: n_windows > 8.
 */
int cgcn_hicinsul_sums(cgcn_stream_t stream, int n, const int32_t *rowptr, const int32_t *col, const double *val,
                       const double *norm, long long n_norm, int n_windows, const int32_t *windows, double *out);

/*
 * A/B compartments: the dense middle between the contact matrix and the eigenvector (chromegcn_amd/compartments.py, whose
 * docstring is the rule).  These five functions are additions to ABI 26 like the functions above:
 * CGCN_ABI_VERSION stays 26, nothing above changes.
 *
 * The dense operands are fp64 and row-major over the m kept bins, 0 <= m <= 8192 (CGCN_ERR_UNSUPPORTED beyond).  B (which
 * becomes M and then Z in place) has m rows of ld doubles: ld >= m, ld even and B on a 16-byte boundary, so that every row can
 * be read in 16-byte pieces (CGCN_ERR_BAD_ARG otherwise); the columns [m, ld) are never read or written.  C is m x m.
 * keep int32 [m]: the kept bins, ascending; rank int32 [n]: the place of a bin in keep, or -1.  A rank outside [0, m), a
 * column outside [0, n) or a kept bin outside [0, n) is passed over, never followed.
 * Every sum is taken in a fixed order -- a wavefront per row or per distance, lane l the terms l, l + 64, ... ascending,
 * one butterfly over the lanes -- without floating-point atomics: the same bits in every run.
 * Enqueue only: no workspace, no allocation, no synchronisation.  CGCN_ERR_BAD_ARG besides: a NULL pointer that would be read
 * or written, a negative size.
 *
 * cgcn_hiccomp_dense: the matrix of cgcn_hicnorm_fill (n bins; rowptr, col, val) scattered into B, which the caller has
 *   zero-filled: B[rank[a] ld + rank[b]] = val[a, b] / (nv[a] * nv[b]) for every stored entry whose two bins are kept, one
 *   fp64 multiplication and one fp64 division; norm fp64 [n_norm] or NULL (val itself) reads as in cgcn_hicinsul_sums.  Each
 *   entry is written once.
 * cgcn_hiccomp_dist_sums: dsum[d] = sum over i with keep[i] + d a kept bin of B[i, rank[keep[i] + d]], d in [0, n); every
 *   entry of dsum fp64 [n] is written.  Zeros of B take part; each unordered pair is met once.
 * cgcn_hiccomp_oe_rows: stages & 1: M[i, j] = B[i, j] / e[d] with d = |keep[j] - keep[i]| where d >= ignore_diags, d < n_e and
 *   e[d] > 0, else 1.0, in place; mean[i] = (sum_j M[i, j]) / m; ss[i] = sum_j (M[i, j] - mean[i])^2.  stages & 2:
 *   Z[i, j] = (M[i, j] - mean[i]) / sqrt(ss[i]) in place from mean and ss as they stand, 0 in a row with ss[i] == 0 (NaN
 *   counts as not above 0).  stages is 1, 2 or 3 (both, in this order).
 * cgcn_hiccomp_corr: C = Z Z^T on v_mfma_f64_16x16x4_f64, K ascending in one accumulator chain per element; an element with
 *   column >= row is stored to both (i, j) and (j, i): C is symmetric bit for bit.
 * cgcn_hiccomp_step: one step of the deflated power iteration, m >= 1: y = C v; dot_p = prev[p] . y for p < n_prev <= 2
 *   (prev fp64 [n_prev][m]; CGCN_ERR_UNSUPPORTED beyond 2); y -= sum_p dot_p prev[p]; lambda = v . y;
 *   rec[0] = lambda, rec[1] = |y|^2, rec[2] = |y - lambda v|^2, rec[3], rec[4] = dot_0, dot_1 (rec fp64 [8]);
 *   v_next = y / |y| (y itself where |y| = 0).  y fp64 [m] is left as deflated; v_next must not be v.
 */
int cgcn_hiccomp_dense(cgcn_stream_t stream, int n, const int32_t *rowptr, const int32_t *col, const double *val,
                       const double *norm, long long n_norm, const int32_t *rank, int m, int ld, double *B);

int cgcn_hiccomp_dist_sums(cgcn_stream_t stream, int n, int m, int ld, const double *B, const int32_t *keep,
                           const int32_t *rank, double *dsum);

int cgcn_hiccomp_oe_rows(cgcn_stream_t stream, int m, int ld, double *B, const int32_t *keep, const double *e, int n_e,
                         int ignore_diags, int stages, double *mean, double *ss);

int cgcn_hiccomp_corr(cgcn_stream_t stream, int m, int ld, const double *Z, double *C);

int cgcn_hiccomp_step(cgcn_stream_t stream, int m, const double *C, const double *v, const double *prev, int n_prev,
                      double *y, double *v_next, double *rec);

/*
 * Chromatin loops after HiCCUPS: pixels enriched over four local backgrounds (chromegcn_amd/loops.py, whose docstring is the
 * rule).  These five functions are additions to ABI 26 like the functions above: CGCN_ABI_VERSION
 * stays 26, nothing above changes.
 *
 * The matrix is what cgcn_hicnorm_fill writes (n bins; rowptr, col, val; vc fp64 [n] its row sums).  band fp64 [n][width] is
 * the raw band, band[i width + d] = A[i, i + d], 0 where i + d >= n.  A pixel is (i, d), 0 <= i < n, 0 <= d <= D, in the order
 * q = i (D + 1) + d, which is ascending (i, j = i + d).  p < w <= 10 are the peak and window half-widths; width >= D + 2 w + 1
 * (CGCN_ERR_BAD_ARG below it: the neighbourhoods of the pixels at distance D reach that far).  norm fp64 [n_norm] or NULL: a
 * bin is valid iff vc > 0 and its norm value is finite, not NaN and not 0 (a bin outside the vector is not valid); expected
 * fp64 [n_expected], n_expected >= min(n, D + 1), is read at the distance of every cell that takes part and reads as 0 beyond
 * its length.  n_chunks <= 64 chunks have the n_chunks - 1 ascending boundaries `bounds` (fp64, device); counts are clipped to
 * W - 1, W <= 65 536.  n (D + 1) must not exceed 2^28.  CGCN_ERR_UNSUPPORTED beyond these limits.
 *
 * cgcn_hicloops_band: fills band from the matrix; the caller has zero-filled it.  Any width >= 1.
 * cgcn_hicloops_pass1: per pixel the sums S, T and the counts C of the four neighbourhoods (donut, lower-left, horizontal,
 *   vertical), each ONE sequential fp64 sum over its cells in row-major (da, db) order; the candidate test (both bins valid,
 *   min_dist <= d, T > 0 and 2 C >= the full size for all four); lambda_x = ((S_x / T_x) * expected[d]) * (nv[i] * nv[j]);
 *   k_x = the number of bounds <= lambda_x (all of them for a NaN).  flags uint32 [n (D + 1)], every entry written: 0, or
 *   1 << 31 | k_v << 18 | k_h << 12 | k_ll << 6 | k_donut for a candidate.  hist int32 [4][n_chunks][W], zeroed by the caller:
 *   hist[x][k_x][min(rint(A[i, j]), W - 1)] += 1 per candidate (integer atomics).  lambda_out fp64 [4][n][D + 1] or NULL: the
 *   four lambda, NaN off the candidates, every entry written.
 * cgcn_hicloops_count: total[0] (int64, device) = the number of enriched pixels: candidates with
 *   min(rint(A[i, j]), W - 1) >= thr[x n_chunks + k_x] for all four x; thr int32 [4][n_chunks] on the device.  It leaves the
 *   per-tile offsets in the workspace for cgcn_hicloops_write, which must be given the same workspace, flags and thr.
 * cgcn_hicloops_write: the enriched pixels in ascending (i, j): pix_ij int32 [capacity][2] = (i, j), pix_val fp64
 *   [capacity][5] = (A[i, j], lambda_donut, lambda_ll, lambda_h, lambda_v), the sums repeated for these pixels alone in pass
 *   1's order (the same bits).  Pixels beyond capacity are dropped.
 *
 * Every sum runs in a fixed order and the only atomics are integer ones: the same bits in every run.  Enqueue only: no
 * allocation, no synchronisation.  CGCN_ERR_BAD_ARG: a NULL pointer that would be read or written, a negative size, w < 1,
 * p outside [0, w), n_chunks < 2, W < 1, norm with n_norm < 1; CGCN_ERR_WORKSPACE: workspace_bytes below
 * cgcn_hicloops_workspace_bytes (0 for an unsupported shape).
 */
int cgcn_hicloops_band(cgcn_stream_t stream, int n, const int32_t *rowptr, const int32_t *col, const double *val, int width,
                       double *band);

int cgcn_hicloops_pass1(cgcn_stream_t stream, int n, int D, int width, const double *band, const double *vc, const double *norm,
                        long long n_norm, const double *expected, long long n_expected, int p, int w, int ignore_diags,
                        int min_dist, const double *bounds, int n_chunks, int W, int32_t *hist, uint32_t *flags,
                        double *lambda_out);

size_t cgcn_hicloops_workspace_bytes(int n, int D);

int cgcn_hicloops_count(cgcn_stream_t stream, int n, int D, int width, const double *band, const uint32_t *flags,
                        const int32_t *thr, int n_chunks, int W, void *workspace, size_t workspace_bytes, long long *total);

int cgcn_hicloops_write(cgcn_stream_t stream, int n, int D, int width, const double *band, const double *vc, const double *norm,
                        long long n_norm, const double *expected, long long n_expected, int p, int w, int ignore_diags,
                        const uint32_t *flags, const int32_t *thr, int n_chunks, int W, long long capacity, void *workspace,
                        size_t workspace_bytes, int32_t *pix_ij, double *pix_val);

/* ---- Pile-ups: aggregate peak analysis of a list of pixel centres (chromegcn_amd/pileup.py holds the rule; DESIGN.md
 * section 4.20).  These four functions are additions to ABI 26 like the functions above: CGCN_ABI_VERSION stays 26, nothing
 * above changes.
 *
 * band fp64 [n][width] is cgcn_hicloops_band's raw band; vc, norm, n_norm and expected, n_expected are read as the loop
 * functions read them (a bin is valid iff vc > 0 and its norm value is finite, not NaN and not 0; expected reads as 0 beyond
 * its length).  w <= 10 is the window half-width, S = 2 w + 1; n width must not exceed 2^28; at most 65 536 groups and 2^24
 * slices.  CGCN_ERR_UNSUPPORTED beyond these limits.
 *
 * cgcn_pileup_values: the value band vband fp64 [n][width], every entry written: for the cell (a, a + dd) the value
 *   A (CGCN_PILEUP_OBSERVED), A / (nv[a] * nv[b]) (CGCN_PILEUP_BALANCED) or (A / (nv[a] * nv[b])) / expected[dd]
 *   (CGCN_PILEUP_OE), in exactly this order; a quiet NaN where a + dd >= n, a bin is not valid, the value is not finite or,
 *   for CGCN_PILEUP_OE, expected[dd] is not > 0.  expected may be NULL for the other two kinds.
 * cgcn_pileup_slices: slice s holds the centres slice_off[s] .. slice_off[s + 1] - 1 (int32 [n_slices + 1], device; at most
 *   256 of them, clipped to that and to n_centres) of ci, cj (int32 [n_centres], device; i < j).  Per slice and offset
 *   (da, db), row-major with da = -w .. w, then db = -w .. w: ONE sequential fp64 sum, from 0.0 and in centre order, of
 *   vband at the cell (i + da, j + db) where that is not NaN, and the int32 count of those cells; both are left in the
 *   workspace for cgcn_pileup_fold.  A centre with i < w, j + w > n - 1, j - i < 2 w or j - i + 2 w >= width adds nothing.
 * cgcn_pileup_fold: the slices group_off[g] .. group_off[g + 1] - 1 (int32 [n_groups + 1], device) belong to group g:
 *   P fp64 [n_groups][S][S] is ONE sequential fp64 sum, from 0.0 and in slice order, of the slice sums; N int64
 *   [n_groups][S][S] the sum of the counts.  Every entry is written; a group without slices gets zeros.  The workspace,
 *   n_slices and w are those of cgcn_pileup_slices.
 *
 * No atomics and a fixed order: the same bits in every run.  Enqueue only: no allocation, no synchronisation.
 * CGCN_ERR_BAD_ARG: a NULL pointer that would be read or written, a negative size, w < 1, width < 1, an unknown kind, norm
 * with n_norm < 1; CGCN_ERR_WORKSPACE: workspace_bytes below cgcn_pileup_workspace_bytes (0 for an unsupported shape).
 */
#define CGCN_PILEUP_OBSERVED 0
#define CGCN_PILEUP_BALANCED 1
#define CGCN_PILEUP_OE 2

int cgcn_pileup_values(cgcn_stream_t stream, int n, int width, const double *band, const double *vc, const double *norm,
                       long long n_norm, const double *expected, long long n_expected, int kind, double *vband);

size_t cgcn_pileup_workspace_bytes(long long n_slices, int w);

int cgcn_pileup_slices(cgcn_stream_t stream, int n, int width, const double *vband, int w, long long n_slices,
                       const int32_t *slice_off, long long n_centres, const int32_t *ci, const int32_t *cj, void *workspace,
                       size_t workspace_bytes);

int cgcn_pileup_fold(cgcn_stream_t stream, int n_groups, int w, long long n_slices, const int32_t *group_off,
                     const void *workspace, size_t workspace_bytes, double *P, long long *N);

/* ---- Two maps compared: the stratum-adjusted correlation coefficient (chromegcn_amd/mapcompare.py holds the rule; DESIGN.md
 * section 4.22).  These three functions are additions to ABI 26 like the functions above: CGCN_ABI_VERSION stays 26, nothing
 * above changes.
 *
 * band fp64 [n][width] is cgcn_hicloops_band's raw band, width >= D + 2 h + 1; h <= 20 is the box half-width; D the largest
 * distance; ld >= n the leading dimension of the strata (the Python layer rounds n up to even).  n width and (D + 1) (ld + 1)
 * must not exceed 2^28: CGCN_ERR_UNSUPPORTED beyond these limits.
 *
 * cgcn_mapcmp_smooth: S fp64 [D + 1][ld], every entry written: S[d][i] = sum over da = -h .. h of R_da, R_da = sum over
 *   db = -h .. h of V(i + da, i + d + db), both plain sequential fp64 sums from 0.0 in ascending order.  V(p, q) is the value
 *   of the cell (min(p, q), max(p, q)), band / (nv[p] * nv[q]) with a norm vector (NaN, 0 and the bins beyond n_norm read as
 *   +inf) and band itself with norm NULL; 0 where p or q is outside [0, n).  S[d][i] = 0 where i + d >= n.
 * cgcn_mapcmp_sums: the sums per stratum d = 0 .. D of the cells (i, i + d) with valid[i] and valid[i + d] (uint8 [n], device)
 *   and Sa[d][i] != 0 or Sb[d][i] != 0; no cell of a stratum below min_dist takes part.  The rows 0 .. n - d - 1 are cut into
 *   chunks of 2048; lane l of 64 adds the rows c0 + l, c0 + l + 64, ... of its chunk in ascending order from 0.0, the lanes
 *   are added by the xor butterfly 32 .. 1, and the chunks' sums are added in chunk order from 0.0.  pass_no = 1 writes
 *   cells int64 [D + 1] and the rows 0 .. 3 of stats fp64 [7][D + 1]: sum x, sum y, sum x / cells, sum y / cells.  pass_no = 2
 *   reads the rows 2 and 3 as the means and writes the rows 4 .. 6: sum (x - mx)^2, sum (y - my)^2, sum (x - mx)(y - my), every
 *   difference, product and sum rounded on its own.  The partial sums live in the workspace.
 *
 * No atomics and a fixed order: the same bits in every run.  Enqueue only: no allocation, no synchronisation.
 * CGCN_ERR_BAD_ARG: a NULL pointer that would be read or written, a negative size, width < D + 2 h + 1, ld < n, a pass_no that is
 * neither 1 nor 2, norm with n_norm < 1; CGCN_ERR_WORKSPACE: workspace_bytes below cgcn_mapcmp_workspace_bytes (0 for an
 * unsupported shape).
 */
int cgcn_mapcmp_smooth(cgcn_stream_t stream, int n, int D, int h, int width, const double *band, const double *norm,
                       long long n_norm, int ld, double *S);

size_t cgcn_mapcmp_workspace_bytes(int n, int D);

int cgcn_mapcmp_sums(cgcn_stream_t stream, int n, int D, int ld, const double *Sa, const double *Sb, const uint8_t *valid,
                     int min_dist, int pass_no, void *workspace, size_t workspace_bytes, long long *cells, double *stats);

#ifdef __cplusplus
}
#endif
#endif /* CHROMEGCN_H */
