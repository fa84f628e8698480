/*
 * hrec.h — C-ABI of libhrec.so, the MI355X (gfx950) hot path of the hybrid
 * ALS + two-tower recommender.
 *
 * The reference (HSoumi/hybrid-als-twotower-recommender) has no FFI of its
 * own: its hot path sits behind two third-party engines that its Python
 * wrappers call. Each entry point below replaces one of those downward calls
 * (file:line into the reference tree):
 *
 *   Spark  ALS.fit            src/als_model.py:52-62   -> hrec_synth_* (data),
 *                                                          hrec_als_init_factors,
 *                                                          hrec_als_half_sweep
 *   Spark  ALSModel.transform src/als_model.py:71-76   -> hrec_als_score
 *   Spark  ALSModel.transform on a pair frame /
 *          RegressionEvaluator (no reference line)    -> hrec_als_predict_pairs,
 *                                                          hrec_als_pair_metrics
 *   Spark  ALSModel.recommendForAllUsers / Items /
 *          UserSubset / ItemSubset (no ref. line)     -> hrec_als_score_topk_pruned
 *          the same minus a training frame's pairs    -> hrec_als_score_topk_pruned_excluding,
 *                                                          hrec_als_score_topk_excluding,
 *                                                          hrec_mask_rows_f32
 *   Spark  RankingEvaluator / RankingMetrics
 *          (no reference line)                        -> hrec_ranking_metrics
 *   Python/sklearn fusion     src/hybrid_system.py:57-75,108 -> hrec_fuse_topk
 *          the same for many users, minus seen pairs
 *          (no reference line)                        -> hrec_hybrid_lists
 *   Python evaluate_individual_models (F1@10 per model chooses the user's
 *          weights) src/hybrid_system.py:42-55, for many
 *          users                                       -> hrec_hybrid_model_f1,
 *                                                          hrec_hybrid_lists_rowwise
 *   Python RecommenderEvaluator (Precision@k / Recall@k, NDCG, MAE, RMSE
 *          per user) src/evaluation.py:19-149, for many
 *          users                                       -> hrec_user_metrics
 *   Beyond-accuracy list measures (coverage, Gini, novelty, diversity,
 *          unexpectedness; no reference line)          -> hrec_row_inv_norms,
 *                                                          hrec_list_quality
 *   Greedy MMR re-ranking of a candidate pool
 *          (no reference line)                        -> hrec_mmr_rerank
 *   ALS predictions explained by the user's history
 *          (no reference line)                        -> hrec_als_explain
 *   Cosine neighbours of rows of one matrix
 *          src/als_model.py:93-104 (factors, towers)  -> hrec_cosine_items,
 *                                                          hrec_cosine_topk
 *   Keras  two-tower graph   src/two_tower_model.py:38-89 -> hrec_tt_*
 *   Keras  fit of one user-embedding row, everything else
 *          frozen, for new users (no reference line)  -> hrec_tt_fold_in_users
 *   Keras  Dot + sorted(...)[:k] for many users        -> hrec_dot_topk
 *          the same minus a training frame's pairs
 *          (no reference line)                        -> hrec_dot_topk_excluding
 *
 * Conventions (all functions):
 *   - every pointer is a DEVICE pointer owned by the caller, except where a
 *     parameter is documented as host memory;
 *   - row-major storage; factor matrices have a leading dimension `kp`
 *     (16, 32, 64, 96, 128, 192 or 256) >= k whose padding columns are kept
 *     at zero (kp > 64: one workgroup per row, csrc/als_wide.hip);
 *   - CSR: int64 indptr[n_rows+1] (local, starts at 0), int32 indices,
 *     f32 values;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *     calls are asynchronous on it and never allocate or synchronise;
 *   - return 0 on success, a negative HREC_E* code on failure; the message
 *     of the last failure on the calling thread is hrec_last_error().
 */
#ifndef HREC_H
#define HREC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: hrec_fuse_topk gained out_minmax; hrec_hybrid_scores gained n_als_rows.
 * 3: hrec_hybrid_minmax / hrec_hybrid_topk removed (the pruned hybrid
 *    replaces them); hrec_dot_topk's +inf bound admits scores >= +inf.
 * 4: the RCCL exchange steps (hrec_comm_*, hrec_allgather, hrec_allreduce_minmax).
 * 6: hrec_als_score_topk_pruned_counts, hrec_cold_fallback*; the pruned ALS
 *    bound is 2^-7 + 2^-13 and its top_k <= 8 results are exact without a
 *    host-side fallback.
 * 7: hrec_encode_ids_ex (the ids' order from the marking pass). */
#define HREC_ABI_VERSION 7

#define HREC_OK 0
#define HREC_E_INVALID (-1) /* bad argument (shape, null pointer, range) */
#define HREC_E_LAUNCH (-2)  /* HIP launch/runtime error                  */
#define HREC_E_UNSUPPORTED (-3)

int hrec_abi_version(void);
const char* hrec_last_error(void);

/* ---------------------------------------------------------------- synth --
 * Synthetic interaction matrix R: (u,i) in R  <=>
 *   h64(seed,u,i) < threshold,  rating(u,i) = h64(seed2,u,i) mod n_levels,
 * h64(s,u,i) = mix64(s*0x9E3779B97F4A7C15 + (u<<32 | i)), mix64 = splitmix64
 * finaliser. The same predicate generates CSR rows (users, transposed=0) and
 * CSC columns (items, transposed=1) independently, so shards agree.
 * Rows are row_begin .. row_begin+n_rows-1 of the chosen orientation; the
 * other dimension has n_cols entries. Replaces the dataset the reference
 * reads at src/data_preprocessing.py:22-35 for the perf configurations. */
int hrec_synth_row_counts(uint64_t seed, uint64_t threshold, int64_t row_begin,
                          int64_t n_rows, int64_t n_cols, int transposed,
                          int64_t* counts, void* stream);
int hrec_synth_fill(uint64_t seed, uint64_t seed2, uint64_t threshold,
                    int64_t row_begin, int64_t n_rows, int64_t n_cols,
                    int transposed, int n_levels, const int64_t* indptr,
                    int32_t* indices, float* values, void* stream);

/* Exclusive prefix sum of counts[n] into out[n+1] (out[n] = total).
 * Workspace: hrec_scan_workspace_bytes(n) bytes of device memory. */
size_t hrec_scan_workspace_bytes(int64_t n);
int hrec_exclusive_scan_i64(const int64_t* counts, int64_t n, int64_t* out,
                            void* workspace, size_t workspace_bytes,
                            void* stream);

/* --------------------------------------------------------------- ingest --
 * The DataFrame -> CSR/CSC step of ALSModel.train (src/als_model.py:51-62:
 * Spark keys factors by the integer ids and keeps duplicate (user, item)
 * ratings as separate terms).
 *
 * hrec_minmax_i64: out[0] = min(x), out[1] = max(x) (device), n >= 1.
 * Workspace: hrec_minmax_i64_workspace_bytes(n). */
size_t hrec_minmax_i64_workspace_bytes(int64_t n);
int hrec_minmax_i64(const int64_t* x, int64_t n, int64_t* out, void* workspace,
                    size_t workspace_bytes, void* stream);

/* hrec_encode_ids: ids[n] (int64, id_lo <= ids <= id_hi) -> uniq[*n_uniq]
 * ascending distinct ids and codes[n] (int32 index into uniq), i.e.
 * numpy.unique(ids, return_inverse=True). *n_uniq is written on the device.
 * A range id_hi - id_lo < 2^31 sorts 32-bit keys on only the bits it spans;
 * pass INT64_MIN, INT64_MAX when the range is unknown. n < 2^31.
 * Workspace: hrec_encode_ids_workspace_bytes(n). */
size_t hrec_encode_ids_workspace_bytes(int64_t n);
int hrec_encode_ids(const int64_t* ids, int64_t n, int64_t id_lo, int64_t id_hi,
                    int64_t* uniq, int64_t* n_uniq, int32_t* codes,
                    void* workspace, size_t workspace_bytes, void* stream);
/* The same, plus *descending (device int32, may be null) = 1 if some
 * ids[i] > ids[i+1], else 0 — hrec_rows_descending_pairs of the codes
 * (the code map is monotone), read by the dense paths' marking pass instead
 * of a pass over the codes — and, when descending is 0, starts[0..n_uniq]
 * (may be null; room for min(n, id_hi - id_lo + 1) + 1 entries) = the CSR
 * row pointer of rows = codes, written by the code pass: ratings grouped by
 * user need neither hrec_rows_descending_pairs nor hrec_coo_to_csr_sorted
 * (the CSR is (starts, item codes, ratings)). starts needs descending. */
int hrec_encode_ids_ex(const int64_t* ids, int64_t n, int64_t id_lo, int64_t id_hi,
                       int64_t* uniq, int64_t* n_uniq, int32_t* codes,
                       int32_t* descending, int64_t* starts, void* workspace,
                       size_t workspace_bytes, void* stream);

/* hrec_coo_to_csr: (rows[nnz], cols[nnz], vals[nnz]) with 0 <= rows < n_rows
 * -> indptr[n_rows+1], indices[nnz], values[nnz]; rows ascending, the entries
 * of a row in input order (numpy.argsort(rows, kind="stable")). The CSC is
 * the same call with rows and cols swapped. nnz, n_rows < 2^31. The entries
 * ride the radix sort as 64-bit (col, rating) values (no gather after it).
 * Workspace: hrec_coo_to_csr_workspace_bytes(nnz, n_rows). */
size_t hrec_coo_to_csr_workspace_bytes(int64_t nnz, int64_t n_rows);
int hrec_coo_to_csr(const int32_t* rows, const int32_t* cols, const float* vals,
                    int64_t nnz, int64_t n_rows, int64_t* indptr, int32_t* indices,
                    float* values, void* workspace, size_t workspace_bytes,
                    void* stream);
/* The same CSR when rows[] is already non-decreasing (then input order is the
 * stable order): entries copied, indptr from the rows, no sort or workspace.
 * indices == cols and values == vals (both or neither) skip the copy: the
 * CSR's column and value arrays are then the input columns themselves.
 * hrec_rows_descending_pairs writes *out (device int32) = 1 if some
 * rows[i] > rows[i+1], else 0 — the caller's choice between the two. */
int hrec_rows_descending_pairs(const int32_t* rows, int64_t n, int32_t* out, void* stream);
int hrec_coo_to_csr_sorted(const int32_t* rows, const int32_t* cols, const float* vals,
                           int64_t nnz, int64_t n_rows, int64_t* indptr, int32_t* indices,
                           float* values, void* stream);

/* hrec_remap_i32: x[i] = table[x[i]] in place (ids outside [0, table_n)
 * -> -1). Maps an ALS shard's column ids (global user / item rows) to rows
 * of an nnz-balanced, padded factor layout (src/als_engine.py RowLayout;
 * Spark partitions users/items into numUserBlocks/numItemBlocks blocks
 * [ext: ALS.scala] — here contiguous row ranges balanced by ratings). */
int hrec_remap_i32(int32_t* x, int64_t n, const int32_t* table, int64_t table_n, void* stream);

/* ------------------------------------------------------------------ ALS --
 * Initial factors (Spark ALS.initialize [ext: pyspark 3.5.1 ALS.scala]:
 * per row a Gaussian-like vector, L2-normalised, f32). Counter-based on
 * (seed, global row) so every shard layout yields the same matrix. */
int hrec_als_init_factors(uint64_t seed, int64_t row_begin, int64_t n_rows,
                          int k, int kp, float* out, void* stream);

/* One ALS half-sweep (Spark computeFactors + NormalEquation.add +
 * CholeskySolver.solve [ext]; called from src/als_model.py:62):
 * for every local dst row r with n_r = indptr[r+1]-indptr[r] ratings,
 *   (sum_j v_j v_j^T + reg_param*n_r*I) x_r = sum_j rating_j v_j,
 * v_j = src_factors[indices[j]], accumulated in f64 (accum_mode 0), solved
 * by Cholesky in f64, stored as f32 in dst_factors[r*kp .. +kp).
 * Rows with n_r == 0 get a zero vector (Spark has no factor for them).
 * accum_mode: 0 = Gramian accumulated in f64 on the f64 matrix cores
 *             (Spark's f64 NormalEquation);
 *             1 = f32 matrix-core products summed in f32 within chunks of 16
 *             ratings, chunks summed in f64 (2x the matrix rate; parity
 *             checked at rtol 1e-4 in tests/test_gpu_core.py). */
int hrec_als_half_sweep(const int64_t* indptr, const int32_t* indices,
                        const float* values, int64_t n_rows,
                        const float* src_factors, int64_t n_src, int k, int kp,
                        double reg_param, int accum_mode, float* dst_factors,
                        void* stream);

/* The same half-sweep with the source factors given in f64
 * (src64[n_src*kp] = the f32 factors converted exactly, hrec_f32_to_f64):
 * identical results, no per-step f32 -> f64 conversion in the gather. For
 * sources that stay in the MI355X's on-chip caches (the user side at
 * BASELINE c2: 100k item rows = 51 MB in f64). kp = 64, accum_mode 0. */
int hrec_als_half_sweep_src64(const int64_t* indptr, const int32_t* indices, const float* values,
                              int64_t n_rows, const double* src64, int64_t n_src, int k, int kp,
                              double reg_param, float* dst_factors, void* stream);
/* The kp = 64, accum_mode 0 half-sweep with the kernel chosen by the caller
 * (the two entries above choose from the launch's shape): kernel 0 = one wave
 * per row, 1 = pooled (one persistent 12-wave workgroup per CU, three waves
 * per SIMD sharing 8 LDS solve slices, rows claimed one by one). Both give
 * the same bits. src: f32 factors (src_f64 = 0) or their f64 copy
 * (src_f64 = 1, 16-B aligned). Additive to ABI 7. */
int hrec_als_half_sweep_kernel(const int64_t* indptr, const int32_t* indices, const float* values,
                               int64_t n_rows, const void* src, int src_f64, int64_t n_src, int k, int kp,
                               double reg_param, int kernel, float* dst_factors, void* stream);
/* out[i] = (double)in[i]. */
int hrec_f32_to_f64(const float* in, int64_t n, double* out, void* stream);

/* Implicit feedback (Spark ALS implicitPrefs = true, confidence weight alpha;
 * ALS.computeFactors, implicit branch [ext]). Additive to ABI 7.
 *
 * hrec_als_gramian: yty[kp*kp] (row-major f64) = sum_s y_s y_s^T over the
 * n_src rows of src_factors[n_src*kp] (f32, converted to f64) — Spark's
 * computeYtY. Zero rows contribute nothing; rows and columns >= k are zero.
 * Slabs of source rows are summed on the f64 matrix cores into per-slab
 * partials in the workspace and the partials in a fixed order: no atomics,
 * the same bits for the same buffer on every call, device and rank.
 * kp = 16, 32 or 64. Workspace: hrec_als_gramian_workspace_bytes(n_src, kp)
 * (0 for an unsupported kp or a negative n_src). */
size_t hrec_als_gramian_workspace_bytes(int64_t n_src, int kp);
int hrec_als_gramian(const float* src_factors, int64_t n_src, int k, int kp,
                     double* yty, void* workspace, size_t workspace_bytes,
                     void* stream);

/* One implicit-feedback half-sweep: for every local dst row r with ratings
 * (j, r_j), v_j = src_factors[indices[j]] in f64 and c1_j = alpha*|r_j|,
 *   A = yty + sum_j c1_j v_j v_j^T,   b = sum_{j: r_j > 0} (1 + c1_j) v_j,
 *   A[d][d] += reg_param * #{j: r_j > 0},   A x_r = b  (f64), stored as f32.
 * yty = hrec_als_gramian of the same src_factors. Rows without ratings and
 * rows whose ratings are all <= 0 get a zero vector; a rating of 0 adds
 * nothing; duplicate entries stay separate terms. alpha >= 0; kp = 16, 32
 * or 64 (rank <= 64), f64 accumulation of f32 sources only. */
int hrec_als_half_sweep_implicit(const int64_t* indptr, const int32_t* indices, const float* values,
                                 int64_t n_rows, const float* src_factors, int64_t n_src, int k, int kp,
                                 double reg_param, double alpha, const double* yty, float* dst_factors,
                                 void* stream);

/* One non-negative half-sweep (Spark ALS nonnegative = true: NNLSSolver in
 * place of CholeskySolver [ext]). Additive to ABI 7. The normal equations of
 * every local dst row are those of hrec_als_half_sweep (implicit = 0: A =
 * sum_j v_j v_j^T + reg_param*n*I, b = sum_j r_j v_j) or of
 * hrec_als_half_sweep_implicit (implicit = 1, with alpha and yty =
 * hrec_als_gramian of the same src_factors); the row is then
 *   argmin_{x >= 0} x^T A x / 2 - b^T x
 * by Spark's mllib NNLS.solve: projected gradients with conjugate-gradient
 * directions from x = 0 in f64, at most max(400, 20 k) iterations, stored as
 * f32. Every entry is >= 0; padding columns are 0. Rows without ratings
 * (implicit: without a rating > 0) get a zero vector. yty must be non-null
 * when implicit is 1 and is ignored otherwise. iters_out: NULL, or
 * int32[n_rows] that receives each row's iteration count (0 for skipped
 * rows). alpha >= 0; kp = 16, 32 or 64 (rank <= 64), f64 accumulation of f32
 * sources only. */
int hrec_als_half_sweep_nonneg(const int64_t* indptr, const int32_t* indices, const float* values,
                               int64_t n_rows, const float* src_factors, int64_t n_src, int k, int kp,
                               double reg_param, int implicit, double alpha, const double* yty,
                               float* dst_factors, int32_t* iters_out, void* stream);

/* out[c*ld_out + r] = in[r*cols + c] (f32), ld_out >= rows. */
int hrec_transpose_f32(const float* in, int64_t rows, int64_t cols, float* out,
                       int64_t ld_out, void* stream);

/* ALS scoring (Spark ALSModel.transform predict UDF [ext], reached from
 * src/als_model.py:75): out[b*n_items + j] = sum_{c<k} U[u_b][c]*V[i_j][c]
 * as a sequential f32 chain, product rounded then sum rounded (no FMA),
 * exactly the JVM loop. NaN where u_b < 0 or i_j < 0 (unknown id).
 * user_factors is [*, kp] row-major; item_factors_t is the TRANSPOSED item
 * matrix [kp, ld_items]; item_rows == NULL means i_j = j. */
int hrec_als_score(const float* user_factors, const int64_t* user_rows,
                   int n_users, const float* item_factors_t, int64_t ld_items,
                   const int64_t* item_rows, int64_t n_items, int k, int kp,
                   float* out, void* stream);

/* ALS predictions for a list of pairs (Spark ALSModel.transform on a frame
 * of (user, item) rows, and RegressionEvaluator over it). Additive to ABI 7.
 *
 * hrec_als_predict_pairs: out[p] = sum_{c<k} U[user_rows[p]][c] *
 * V[item_rows[p]][c], p < n: the chain of hrec_als_score (f32, sequential in
 * c from 0.0f, product rounded then sum rounded), so a pair gets the bits the
 * score matrix holds for it. Both factor matrices are row-major [n_rows, kp]
 * (the item matrix is NOT transposed here), 16-B aligned. A row index
 * outside [0, n_rows) on either side (any negative value marks an unknown
 * id) gives a quiet NaN and is never dereferenced. n == 0 is a no-op.
 *
 * hrec_als_pair_metrics: the same predictions (stored when pred_out is not
 * NULL) and, over the pairs whose prediction is not NaN, with y = labels[p],
 * p^ = (double)prediction and e = y - p^ in f64, sums_out[HREC_PAIR_SUMS]
 * (device f64) as named below; HREC_PAIR_N_NAN counts the pairs with a NaN
 * prediction (unknown row or a NaN chain), which enter no sum. No
 * floating-point atomics: per-block partials in the workspace (the block
 * count depends on n alone) are added in a fixed order by a second launch,
 * so equal inputs give equal bits on every call. n == 0 writes zeros.
 * Workspace: hrec_als_pair_metrics_workspace_bytes(n). */
#define HREC_PAIR_N_OK 0      /* pairs with a prediction (as f64, exact) */
#define HREC_PAIR_N_NAN 1     /* pairs with a NaN prediction             */
#define HREC_PAIR_SUM_E 2     /* sum e                                   */
#define HREC_PAIR_SUM_ABS_E 3 /* sum |e|                                 */
#define HREC_PAIR_SUM_E2 4    /* sum e^2                                 */
#define HREC_PAIR_SUM_Y 5     /* sum y                                   */
#define HREC_PAIR_SUM_Y2 6    /* sum y^2                                 */
#define HREC_PAIR_SUM_P 7     /* sum p^                                  */
#define HREC_PAIR_SUM_P2 8    /* sum p^^2                                */
#define HREC_PAIR_SUM_YP 9    /* sum y p^                                */
#define HREC_PAIR_SUMS 10
int hrec_als_predict_pairs(const float* user_factors, int64_t n_user_rows,
                           const float* item_factors, int64_t n_item_rows, int k, int kp,
                           const int64_t* user_rows, const int64_t* item_rows, int64_t n,
                           float* out, void* stream);
size_t hrec_als_pair_metrics_workspace_bytes(int64_t n);
int hrec_als_pair_metrics(const float* user_factors, int64_t n_user_rows,
                          const float* item_factors, int64_t n_item_rows, int k, int kp,
                          const int64_t* user_rows, const int64_t* item_rows, int64_t n,
                          const double* labels, float* pred_out, double* sums_out,
                          void* workspace, size_t workspace_bytes, void* stream);

/* Spark 3.5 RankingMetrics with binary relevance over ranked id lists on the
 * device (RankingEvaluator: precisionAtK, recallAtK, meanAveragePrecision,
 * meanAveragePrecisionAtK, ndcgAtK). Additive to ABI 7.
 *
 * pred[r * pred_ld + i], i < len_r, is row r's list, best first; len_r =
 * pred_len ? pred_len[r] (clamped to [0, pred_len_max]) : pred_len_max, with
 * 0 <= pred_len_max <= 1024 and pred_ld >= pred_len_max; entries at i >= len_r
 * are never read. Ids are raw int64 keys, any value is legal.
 * labels[label_indptr[r] .. label_indptr[r + 1]) is row r's ground truth,
 * sorted ascending; duplicates count once (Spark's lab.toSet): m_r distinct
 * labels. 1 <= k <= 1024. gain[i] = 1 / ln(i + 2), i < k, and idcg[j] =
 * gain[0] + ... + gain[j - 1], j <= k (k + 1 entries, idcg[0] = 0), are made
 * by the caller on the host, so no device logarithm decides a bit.
 *
 * Per row, f64, hit(i) = pred[i] in labels, cnt(i) = hits at positions <= i:
 *   precision = #{i < min(len, k): hit} / k     recall = the same count / m
 *   AP    = sum_{hit i < len} cnt(i) / (i + 1), ascending i,  / m
 *   AP@k  = the same over i < min(k, len),                    / min(m, k)
 *   NDCG@k: n = min(max(len, m), k); sum_{hit i < min(n, len)} gain[i],
 *           ascending i,                                      / idcg[min(m, n)]
 * m = 0: all five are 0 and the row counts in HREC_RANK_N_EMPTY. per_row
 * (optional, [n_rows][5] in this order) receives them; sums_out[HREC_RANK_SUMS]
 * (device f64) the totals named below. *unsorted (device int32, written by the
 * call) is 1 when some label row has a descending neighbour pair (the sums
 * are then meaningless), else 0. No floating-point atomics: per-block
 * partials in the workspace (the block count depends on n_rows alone), added
 * in a fixed order by a second launch, so equal inputs give equal bits on
 * every call. n_rows == 0 writes zeros.
 * Workspace: hrec_ranking_metrics_workspace_bytes(n_rows). */
#define HREC_RANK_N_ROWS 0        /* rows (users) seen, as f64, exact            */
#define HREC_RANK_N_EMPTY 1       /* rows with an empty label set (all metrics 0)*/
#define HREC_RANK_HITS 2          /* sum over rows of hits within the first k    */
#define HREC_RANK_SUM_PRECISION 3
#define HREC_RANK_SUM_RECALL 4
#define HREC_RANK_SUM_AP 5        /* Spark meanAveragePrecision terms            */
#define HREC_RANK_SUM_AP_K 6      /* meanAveragePrecisionAt(k) terms             */
#define HREC_RANK_SUM_NDCG 7
#define HREC_RANK_SUMS 8
size_t hrec_ranking_metrics_workspace_bytes(int64_t n_rows);
int hrec_ranking_metrics(const int64_t* pred, int64_t pred_ld, int pred_len_max, const int32_t* pred_len,
                         const int64_t* label_indptr, const int64_t* labels, int64_t n_rows, int k,
                         const double* gain, const double* idcg, double* per_row, double* sums_out,
                         int32_t* unsorted, void* workspace, size_t workspace_bytes, void* stream);

/* Scoring consumed by a top-k, for whole item ranges (no id gather): the
 * same JVM-exact f32 dot as hrec_als_score for every (user, item j < n_items)
 * pair, but the B x n_items score matrix is never written: the top_k-th
 * best score of the first 2048 items bounds each user's final top_k-th score
 * from below, a fused pass keeps only pairs at or above that bound, and an
 * exact stable top-k runs over the survivors. out_idx/out_val: [n_users,
 * min(top_k, n_items)]. *overflow (device int) is set to 1 when some user had
 * more than 4096 survivors (ties/adversarial scores): the result is then
 * incomplete and the caller must fall back to hrec_als_score + hrec_topk_f32.
 * Users must be known (user_rows >= 0). ld_items % 4 == 0. */
size_t hrec_als_score_topk_workspace_bytes(int n_users, int64_t n_items, int top_k);
int hrec_als_score_topk(const float* user_factors, const int64_t* user_rows,
                        int n_users, const float* item_factors_t, int64_t ld_items,
                        int64_t n_items, int k, int kp, int top_k, int64_t* out_idx,
                        float* out_val, int* overflow, void* workspace,
                        size_t workspace_bytes, void* stream);

/* hrec_als_score_topk over the items a query has not seen: the same chain
 * over every pair, the same stable ranking, with the items of the query's
 * exclusion set deleted from it (the left-anti join of the recommendations
 * against a training frame). Additive to ABI 7.
 *
 * excl_indptr / excl_cols: a CSR over the factor rows of the query side; the
 * set of query b is excl_cols[excl_indptr[r] .. excl_indptr[r + 1]) with r =
 * user_rows[b], so one CSR serves every batch and subset. A row's columns are
 * ascending; duplicates count once; a column outside [0, n_items) is ignored
 * and never used as an index. out_len[b] (int32, device) = min(kk, n_items -
 * distinct in-range excluded columns of b), kk = min(top_k, n_items); the
 * entries of out_idx / out_val at positions >= out_len[b] are unspecified.
 * The bound of hrec_als_score_topk is taken over the sample's items that
 * stay (excluded sample scores are set to -inf first; a query with fewer
 * than kk of them left gets -inf and keeps every item), the filter pass is
 * the same, and the excluded candidates are taken out of the lists (NaN
 * scores, ranked last) before the final top-k. *overflow as there: some query
 * had more than 4096 candidates, excluded ones included; the result is
 * incomplete and the caller falls back to hrec_als_score + hrec_mask_rows_f32
 * (fill NaN) + hrec_topk_f32. Same limits on top_k, kp, ld_items and n_users;
 * users must be known. The workspace is hrec_als_score_topk's. */
size_t hrec_als_score_topk_excluding_workspace_bytes(int n_users, int64_t n_items, int top_k);
int hrec_als_score_topk_excluding(const float* user_factors, const int64_t* user_rows, int n_users,
                                  const float* item_factors_t, int64_t ld_items, int64_t n_items, int k,
                                  int kp, int top_k, const int64_t* excl_indptr, const int32_t* excl_cols,
                                  int64_t* out_idx, float* out_val, int32_t* out_len, int* overflow,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* The masking step of hrec_als_score_topk_excluding on a score matrix:
 * vals[i * row_stride + c] = fill for every column c in [0, n) of the
 * exclusion set of factor row row_ids[i] (a negative row id: the empty set);
 * kept_out[i] (int32) = n - distinct in-range excluded columns. n and n_rows
 * below 2^31, row_stride >= n. Additive to ABI 7. Every *_excluding entry
 * reads its CSR by this convention (device side: csrc/exclusion.h). */
int hrec_mask_rows_f32(float* vals, int64_t n_rows, int64_t n, int64_t row_stride, const int64_t* row_ids,
                       const int64_t* excl_indptr, const int32_t* excl_cols, float fill,
                       int32_t* kept_out, void* stream);

/* Pruned form of hrec_als_score_topk (same outputs, same overflow contract):
 * the sample bound thr_b as there, then a bf16 matrix-core filter keeps
 * every item with approx score >= thr_b - E, E = (2^-7 + 2^-13) ||u|| max
 * ||v|| + 1e-30 (bounds |bf16 dot - JVM chain| for k <= 256: 2^-8 relative
 * rounding per bf16 operand), and the JVM chain over those items alone
 * leaves exactly the fused filter's survivors (score >= thr_b), ranked by the
 * same stable top-k. *overflow is also set when a bound is not finite (a
 * non-finite factor), when the bf16 filter's list overflows, or when a known
 * user ends with fewer than min(top_k, n_items) candidates (a bound slip:
 * never short or padded ids). For min(top_k, n_items) <= 8 a set *overflow
 * is resolved in the same call, on the device (a gated exact top-k of the
 * JVM chain over every item, no host round trip): the outputs are then
 * always exact and *overflow only reports that the fallback ran; above 8 the
 * caller falls back as for hrec_als_score_topk. items_bf16: hrec_als_items_bf16 of
 * item_factors (row-major [n_items, ld_v], the same values as
 * item_factors_t), 256-B aligned; it is built once per item matrix.
 * hrec_als_score_topk_pruned_counts copies the last call's diagnostics from
 * its workspace: out[0 .. n) = pairs the bf16 bound kept per user,
 * out[n .. 2n) = candidates per user (int32, device); zeros when the call
 * took the small-catalogue (fused) path. */
size_t hrec_als_items_bf16_bytes(int64_t n_items, int k);
int hrec_als_items_bf16(const float* item_factors, int64_t ld_v, int64_t n_items, int k,
                        void* out, size_t out_bytes, void* stream);
size_t hrec_als_score_topk_pruned_workspace_bytes(int n_users, int64_t n_items, int top_k, int k);
int hrec_als_score_topk_pruned(const float* user_factors, const int64_t* user_rows, int n_users,
                               const float* item_factors_t, int64_t ld_items,
                               const float* item_factors, int64_t ld_v, const void* items_bf16,
                               int64_t n_items, int k, int kp, int top_k, int64_t* out_idx,
                               float* out_val, int* overflow, void* workspace,
                               size_t workspace_bytes, void* stream);
int hrec_als_score_topk_pruned_counts(const void* workspace, int n_users, int64_t n_items, int top_k, int k,
                                      int32_t* out, void* stream);

/* hrec_als_score_topk_pruned over the items a query has not seen: the
 * answer of hrec_als_score_topk_excluding (the full stable ranking, the
 * query's excluded entries deleted, cut to kk = min(top_k, n_items); out_len[b]
 * = min(kk, n_items - distinct in-range excluded columns of b); entries at
 * positions >= out_len[b] unspecified) with the bf16 matrix-core bound in
 * front of the exact chain. Additive to ABI 7. The exclusion CSR and out_len
 * are those of hrec_als_score_topk_excluding, the operands and their checks
 * those of hrec_als_score_topk_pruned.
 *
 * The bound is taken over the sample's items that stay: the bf16 scores of
 * the first min(n_items, 8192) items are materialised at every top_k, the
 * query's excluded ones set to -inf, and t_b is the kk-th of the 64 lane
 * maxima (kk <= 64) or the kk-th best (above) of the rest: kk non-excluded
 * items have chain >= t_b - E = tau_b, so the kk-th best non-excluded chain is
 * >= tau_b. The filter at tau_b - E and the exact chain are unchanged (they
 * also keep excluded items that reach the bound); the excluded candidates
 * leave before the ranking (kk <= 8: inside the fused rescore-and-rank
 * kernel; above: NaN scores, ranked last).
 *
 * *overflow: as for hrec_als_score_topk_pruned, and also when a query has
 * fewer than kk non-excluded items among the sample's lane maxima / items
 * (t_b = -inf: no bound). Nothing is resolved on the device here: a set
 * *overflow means the answer is incomplete at every top_k, and the caller
 * falls back to hrec_als_score_topk_excluding (and from there as it says).
 * n_items <= 2048 takes hrec_als_score_topk_excluding itself; the workspace
 * query returns the larger of the two needs. hrec_als_score_topk_pruned_counts
 * reads this call's workspace too (for kk <= 8 the candidates are counted
 * after the exclusion, above 8 before it). */
size_t hrec_als_score_topk_pruned_excluding_workspace_bytes(int n_users, int64_t n_items, int top_k, int k);
int hrec_als_score_topk_pruned_excluding(const float* user_factors, const int64_t* user_rows, int n_users,
                                         const float* item_factors_t, int64_t ld_items,
                                         const float* item_factors, int64_t ld_v, const void* items_bf16,
                                         int64_t n_items, int k, int kp, int top_k,
                                         const int64_t* excl_indptr, const int32_t* excl_cols,
                                         int64_t* out_idx, float* out_val, int32_t* out_len, int* overflow,
                                         void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- top-k --
 * Stable descending top-k of each of n_rows rows (row i starts at
 * vals + i*row_stride, n elements): larger value first, equal values keep
 * input order (smaller index first), NaN last — Python's
 * sorted(..., key=score, reverse=True)[:k] as used at
 * src/hybrid_system.py:108 and src/als_model.py:173. Any top_k >= 1 (clamped
 * to n): up to 1024 by segment selections, above by a stable per-row radix
 * sort on the device (then n_rows * n < 2^31). */
size_t hrec_topk_workspace_bytes(int64_t n_rows, int64_t n, int top_k, int is_f64);
int hrec_topk_f32(const float* vals, int64_t n_rows, int64_t n, int64_t row_stride,
                  int top_k, int64_t* out_idx, float* out_val, void* workspace,
                  size_t workspace_bytes, void* stream);
int hrec_topk_f64(const double* vals, int64_t n_rows, int64_t n, int64_t row_stride,
                  int top_k, int64_t* out_idx, double* out_val, void* workspace,
                  size_t workspace_bytes, void* stream);

/* --------------------------------------------------------------- fusion --
 * HybridRecommendationSystem.adaptive_fusion + top-k
 * (src/hybrid_system.py:57-75 and :108): both score vectors (aligned to the
 * same item order) are min-max scaled with sklearn MinMaxScaler arithmetic
 * in their own dtype (als f64; tt f32 when tt_is_f32, else f64), then
 * fused = w0*als_norm + w1*tt_norm in f64 with (w0,w1) = (0.8,0.2) when
 * als_wins (the strict als_f1 > tt_f1 of :69) else (0.2,0.8).
 * out_fused (optional, n doubles) receives every fused score; out_idx /
 * out_score receive the stable top min(top_k, n) (any top_k >= 0; 0 = no
 * top-k). out_minmax (optional, 4 doubles) receives (als min, als max,
 * tt min, tt max): the two scalers' data_min_ / data_max_ after the
 * reference's fit_transform (src/hybrid_system.py:66-67). */
size_t hrec_fuse_workspace_bytes(int64_t n, int top_k);
int hrec_fuse_topk(const double* als, const void* tt, int tt_is_f32, int64_t n,
                   int als_wins, int top_k, int64_t* out_idx, double* out_score,
                   double* out_fused, double* out_minmax, void* workspace,
                   size_t workspace_bytes, void* stream);

/* Batched fusion for many users over one item range (a shard of the item
 * set when the item rows are split across GPUs):
 * hrec_rows_minmax_f32: out[r] = min, out[n_rows + r] = max of row r (NaN
 * ignored) — reduced across shards by the caller (RCCL all-reduce MIN on the
 * first half, MAX on the second);
 * hrec_fuse_rows_topk: per row, MinMaxScaler of the ALS scores in f64 and of
 * the two-tower scores in f32 with the GIVEN (global) row min/max, f64 fusion
 * as hrec_fuse_topk, then the stable top-k of the row; indices are shifted by
 * idx_offset (the shard's first global item). als/tt: [n_rows, ld] f32.
 * hrec_topk_f64_keyed: stable top-k where keys[] (e.g. global item ids, -1 =
 * empty slot) are both the tie-break and the returned ids — the merge of the
 * per-shard candidates. */
int hrec_rows_minmax_f32(const float* x, int64_t n_rows, int64_t n, int64_t ld,
                         float* out, void* stream);
size_t hrec_fuse_rows_workspace_bytes(int64_t n_rows, int64_t n, int top_k);
int hrec_fuse_rows_topk(const float* als, const float* tt, int64_t n_rows, int64_t n,
                        int64_t ld, const float* als_minmax, const float* tt_minmax,
                        int als_wins, int top_k, int64_t idx_offset, int64_t* out_idx,
                        double* out_val, void* workspace, size_t workspace_bytes,
                        void* stream);
int hrec_topk_f64_keyed(const double* vals, const int64_t* keys, int64_t n_rows, int64_t n,
                        int top_k, int64_t* out_idx, double* out_val, void* workspace,
                        size_t workspace_bytes, void* stream);

/* Hybrid ranked lists (additive to ABI 7): for each row r of the f32 score
 * matrices als / tt [n_rows, ld] (ld >= n, n_rows < 65536), the stable
 * descending ranking that hrec_fuse_topk(a_r, tt_r as f32, n, als_wins,
 * top_k = n) gives, with the row's excluded columns deleted, cut to kk =
 * min(top_k, n) (top_k in [1, 1024]): the same indices, out_val bits and
 * out_minmax[r] ([n_rows][4], or NULL). a_rj = als_fallback[j] where
 * als[r][j] is NaN and als_fallback ([n] f64, or NULL) is given, else
 * (double)als[r][j]. Both scalers see every column, excluded ones included;
 * equal fused scores keep column order; NaN fused scores rank last.
 * Exclusion (hrec_mask_rows_f32's convention): row r's set is
 * excl_cols[excl_indptr[q] .. excl_indptr[q + 1]) with q = excl_rows[r] (q <
 * 0: empty), ascending, duplicates counting once, a column outside [0, n)
 * ignored and never used as an index; all three NULL: nothing excluded.
 * out_len[r] = min(kk, n - distinct in-range excluded columns); entries at
 * positions >= out_len[r] are unspecified; an excluded column never appears
 * before out_len[r].
 * mode 0 (bounded): each row's first HREC_HYBRID_LISTS_SAMPLE columns give a
 * lower bound of its kk-th key; the columns reaching it go to a list of
 * HREC_HYBRID_LISTS_CAP entries. *overflow = 1 when some row had more: the
 * answer is then incomplete (rows that fit are still right) and the caller
 * repeats the call with mode 1. n <= HREC_HYBRID_LISTS_SAMPLE never
 * overflows. mode 1 (full): every fused key is written to the workspace and
 * ranked; always complete, *overflow = 0; >= 16 * n_rows * n bytes. */
#define HREC_HYBRID_LISTS_SAMPLE 4096
#define HREC_HYBRID_LISTS_CAP 4096
size_t hrec_hybrid_lists_workspace_bytes(int64_t n_rows, int64_t n, int top_k, int mode);
int hrec_hybrid_lists(const float* als, const float* tt, int64_t n_rows, int64_t n, int64_t ld,
                      const double* als_fallback, int als_wins, int top_k, int mode,
                      const int64_t* excl_rows, const int64_t* excl_indptr,
                      const int32_t* excl_cols, int64_t* out_idx, double* out_val,
                      int32_t* out_len, double* out_minmax, int* overflow, void* workspace,
                      size_t workspace_bytes, void* stream);
/* hrec_hybrid_lists with the fusion weights chosen per row (additive to ABI
 * 7): row r fuses with (0.8, 0.2) when row_wins[r] != 0 and with (0.2, 0.8)
 * otherwise (row_wins: [n_rows] int32, device, not NULL). Everything else —
 * the arguments, their checks, the modes, the outputs' bits and the
 * workspace (hrec_hybrid_lists_workspace_bytes) — is hrec_hybrid_lists'; a
 * constant row_wins gives hrec_hybrid_lists(als_wins = that constant). */
int hrec_hybrid_lists_rowwise(const float* als, const float* tt, int64_t n_rows, int64_t n,
                              int64_t ld, const double* als_fallback, const int32_t* row_wins,
                              int top_k, int mode, const int64_t* excl_rows,
                              const int64_t* excl_indptr, const int32_t* excl_cols,
                              int64_t* out_idx, double* out_val, int32_t* out_len,
                              double* out_minmax, int* overflow, void* workspace,
                              size_t workspace_bytes, void* stream);

/* Per-row, per-model F1@k (additive to ABI 7): the batch form of the
 * reference's evaluate_individual_models, which chooses the fusion weights of
 * one user. als / tt / ld / als_fallback / n_rows as for hrec_hybrid_lists; k
 * in [1, 1024]; mode 0 or 1. Per row r and model, the selection is the first
 * min(k, n) columns of the stable descending ranking of the model's keys
 * (equal keys keep column order, NaN last in column order): ALS keys are the
 * f64 values a_rj of hrec_hybrid_lists, two-tower keys the f32 scores — the
 * order sorted(dict(preds).items(), key=score, reverse=True)[:k] gives
 * predict_for_user's list over a frame of distinct ids. Then, in f64 and in
 * compute_f1_score's operation order: tp = the row's labels found in the
 * selection, p = tp / k (k as passed, also when n < k), r = tp / total,
 * f1 = (p + r > 0) ? 2 * (p * r) / (p + r) : 0.
 * Labels (a CSR shaped like the exclusion CSR): row r's candidate labels are
 * label_cols[label_indptr[q] .. label_indptr[q + 1]) with q = label_rows[r]
 * (q < 0: a row without labels), column indices ascending and distinct;
 * label_total[q] (int32) is the size of the user's whole ground-truth set, >=
 * the number of its labels that are candidates. All four NULL: no row has
 * labels.
 * out_f1 [n_rows][2] = (ALS, two-tower); out_wins [n_rows] = f1_als > f1_tt;
 * out_top (optional) [n_rows][2][min(k, n)] = the two selections' columns. A
 * row with q < 0 or label_total[q] == 0 gets NaN for both F1s and out_wins =
 * (default_wins != 0).
 * mode 0 (bounded): per model, the row's first HREC_HYBRID_LISTS_SAMPLE
 * columns give a lower bound of the selection's last key; one pass over both
 * matrices appends the columns reaching it to a list of
 * HREC_HYBRID_LISTS_CAP entries per row and model. *overflow = 1 when some
 * list had more: the answer is then incomplete and the caller repeats the
 * call with mode 1. n <= HREC_HYBRID_LISTS_SAMPLE never overflows. mode 1
 * (full): both key rows are written to the workspace (>= 16 * n_rows * n
 * bytes) and ranked; always complete, *overflow = 0. */
size_t hrec_hybrid_model_f1_workspace_bytes(int64_t n_rows, int64_t n, int k, int mode);
int hrec_hybrid_model_f1(const float* als, const float* tt, int64_t n_rows, int64_t n, int64_t ld,
                         const double* als_fallback, int k, int mode, const int64_t* label_rows,
                         const int64_t* label_indptr, const int32_t* label_cols,
                         const int32_t* label_total, int default_wins, double* out_f1,
                         int32_t* out_wins, int64_t* out_top, int* overflow, void* workspace,
                         size_t workspace_bytes, void* stream);

/* Per-user evaluation by the reference's own protocol (additive to ABI 7):
 * RecommenderEvaluator's Precision@k / Recall@k, NDCG, MAE and RMSE
 * (src/evaluation.py:19-149) for every row of a batch, from ranked lists and
 * scores that are already on the device. Row r's result is what the per-user
 * methods return for (actual, predicted) with actual = {itemId: rating} of the
 * user's rows in frame order and predicted = the row's scores over the n
 * candidates in candidate order.
 * Lists: ranked[r * ranked_ld + i], i < len_r = list_len ? list_len[r]
 * (clamped to [0, list_n]) : list_n, are row r's candidate columns, best
 * first: the stable descending ranking of the row's scores (equal scores keep
 * column order, NaN last) cut to min(max k, n) or longer — hrec_hybrid_lists'
 * out_idx, a model's half of hrec_hybrid_model_f1's out_top (ranked_ld = 2 *
 * kk), or a hrec_topk_* result. 0 <= list_n <= 1024, ranked_ld >= list_n; a
 * column outside [0, n) hits nothing.
 * Actual ratings (a CSR shaped like the exclusion CSR): row r's user is q =
 * act_rows[r] (q < 0, or all five pointers NULL: a row without ratings), its
 * segment [act_indptr[q], act_indptr[q + 1]). act_cols holds the candidate
 * column of each rated item, ascending, -1 (first) for an item outside the
 * candidate frame; act_ratings the ratings aligned with act_cols; act_frame
 * the same ratings in frame order. A user's items are distinct.
 *   threshold = the bits of np.mean(ratings in frame order): numpy's pairwise
 *     summation (below 8 terms serial; up to 128 eight interleaved
 *     accumulators combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the
 *     tail; above 128 the recursive halving, the split rounded down to a
 *     multiple of 8), divided by the count;
 *   relevant = the items with threshold - 0.1 <= rating <= threshold + 0.1,
 *     items outside the candidate frame included;
 *   Precision@k = hits / k, Recall@k = hits / |relevant| (0 when empty) with
 *     hits = the relevant items among the first min(k, len_r) list entries,
 *     for each of k_values[n_k] (a HOST array; 1 <= n_k <= 8, k in [1, 1024]);
 *   over the m common items (column in [0, n)), t = rating, p = score:
 *   NDCG@ndcg_k: MinMaxScaler fitted on t (scale = 1 / range, a range below
 *     10 eps -> 1; min_ = 0 - min * scale; x * scale + min_, two roundings)
 *     applied to both sides, grades (x >= 0.33) + (x >= 0.66) (NaN: 2),
 *     sklearn's tie-averaged DCG over the three predicted-grade groups, best
 *     first: (mean true grade of the group) * (disc_cs[end] - disc_cs[begin])
 *     of the positions it occupies; IDCG = 2 * disc_cs[n2] + (disc_cs[n2 +
 *     n1] - disc_cs[n2]) over the true grades' counts; 0 when IDCG is 0.
 *     disc_cs (device, ndcg_k + 1 entries) = 0 followed by the running sums
 *     of 1 / log2(i + 2), i < ndcg_k, made by the caller on the host (indices
 *     past ndcg_k read entry ndcg_k), so no device logarithm decides a bit;
 *   MAE / RMSE: both sides as ((4 * (v - min)) / (max - min)) + 1 over the
 *     common items, MAE = mean |t - p|, RMSE = sqrt(mean (t - p)^2).
 * Score sources (source; scores / ld >= n as [n_rows][ld]):
 *   HREC_UM_SRC_F64    scores: f64 matrix; all arithmetic in f64;
 *   HREC_UM_SRC_F32    scores: f32 matrix with np.float32 semantics (the
 *     two-tower model's): in NDCG f32(f64(p) * scale), then f32(f64(that) +
 *     min_), compared in f64; the 1-5 rescale all in f32, widened before the
 *     subtraction;
 *   HREC_UM_SRC_ALS    scores: the ALS f32 matrix; p = a_rj of
 *     hrec_hybrid_lists (als_fallback[j] where NaN and given), f64;
 *   HREC_UM_SRC_FUSED  scores / tt_scores: both f32 matrices, als_fallback,
 *     minmax = hrec_hybrid_lists' out_minmax rows, row_wins [n_rows] int32:
 *     p = the fused score hrec_hybrid_lists(_rowwise) ranks, recomputed to its
 *     bits, f64.
 * All metric arithmetic is f64 (f32 where stated), unfused.
 * Outputs: per_row [n_rows][2 * n_k + 3] = Precision per k, Recall per k,
 * NDCG, MAE, RMSE; status [n_rows] = the HREC_UM_* bits below. Where the
 * reference raises ValueError the value is NaN and the bit is set: NDCG with
 * exactly one common item (or an infinite score among them), MAE / RMSE when a
 * rescaled value is not finite (one common item, constant ratings, constant
 * scores, a NaN score). No common item: NDCG = MAE = RMSE = 0 as the
 * reference returns. A row without ratings: all zeros, counted nowhere.
 * sums_out [2 * (2 * n_k + 3) + HREC_UM_STATUS_BITS] (device f64): per column
 * the sum over the rows where it is defined, then per column the count of
 * those rows, then the number of rows with each status bit. Per-block
 * partials in the workspace, added in a fixed order by a second launch, no
 * floating-point atomics: equal inputs give equal bits on every call.
 * n_rows < 65536; n_rows == 0 returns HREC_OK and touches nothing.
 * Workspace: hrec_user_metrics_workspace_bytes(n_rows). */
#define HREC_UM_MAX_K 8
#define HREC_UM_SRC_F64 0
#define HREC_UM_SRC_F32 1
#define HREC_UM_SRC_ALS 2
#define HREC_UM_SRC_FUSED 3
#define HREC_UM_NDCG_UNDEFINED 1 /* NDCG is NaN                                  */
#define HREC_UM_ERR_UNDEFINED 2  /* MAE and RMSE are NaN                         */
#define HREC_UM_NO_COMMON 4      /* no rated item among the candidates           */
#define HREC_UM_NO_RELEVANT 8    /* nothing in the band: Recall is 0             */
#define HREC_UM_NO_RATINGS 16    /* a row without ratings                        */
#define HREC_UM_STATUS_BITS 5
size_t hrec_user_metrics_workspace_bytes(int64_t n_rows);
int hrec_user_metrics(const int64_t* ranked, int64_t ranked_ld, int list_n, const int32_t* list_len,
                      int64_t n_rows, int64_t n, const int32_t* k_values, int n_k, int ndcg_k,
                      const double* disc_cs, const int64_t* act_rows, const int64_t* act_indptr,
                      const int32_t* act_cols, const double* act_ratings, const double* act_frame,
                      int source, const void* scores, const float* tt_scores, int64_t ld,
                      const double* als_fallback, const double* minmax, const int32_t* row_wins,
                      double* per_row, int32_t* status, double* sums_out, void* workspace,
                      size_t workspace_bytes, void* stream);

/* The position of every held-out item among ALL candidates (additive to ABI
 * 7): what a top-n list cut at 1024 cannot say. For row r with candidate
 * columns 0 .. n - 1 and scores s_rj from one of hrec_user_metrics' sources
 * (source, scores, tt_scores, ld, als_fallback, minmax, row_wins exactly as
 * there; the fused value is recomputed to its bits), a label entry with
 * column p gets
 *   rank = #{ j : j != p, j not excluded for r, j stands before p }
 * in the order of every top-k here: larger value first, equal values by
 * smaller column first, NaN last (NaNs by column). That is the 0-based
 * position of p in the list hrec_hybrid_lists / hrec_dot_topk_excluding /
 * hrec_als_score_topk_excluding would return for row r if n entries were
 * allowed. Ties are resolved by that order, not counted as 1/2: the AUC below
 * is the AUC of the ranking that is served.
 * Labels (a CSR shaped like the exclusion CSR): row r's entries are
 * label_cols[label_indptr[q] .. label_indptr[q + 1]) with q = label_rows[r]
 * (q < 0, or all three pointers NULL: a row without labels); columns in any
 * order, duplicates allowed, every entry answered. An entry whose column is
 * outside [0, n) (-1: not a candidate) or in the row's exclusion set is
 * unranked: rank -1. label_weight (optional, f64, aligned with label_cols):
 * the entry's weight w, 1 when NULL.
 * Exclusion (optional): (excl_rows, excl_indptr, excl_cols), the triple of
 * hrec_hybrid_lists (columns ascending per row).
 * Outputs: out_rank (optional) int32 aligned with label_cols. out_row_n
 * [n_rows][3] int32 = live (n minus the row's distinct excluded columns in
 * [0, n)), ranked and unranked label entries. out_row [n_rows][4] f64, with h
 * = the row's ranked labels after collapsing duplicate columns, S = the sum of
 * their ranks and L = live, integers in int64 and exactly these f64
 * operations:
 *   auc = 1.0 - (double)(S - h * (h - 1) / 2) / ((double)h * (double)(L - h)),
 *     NaN when h == 0 or L == h;
 *   reciprocal_rank = 1.0 / (double)(1 + min rank), NaN when h == 0;
 *   sum_w_pr = sum of w_p * ((double)rank_p / (double)(L - 1)) over the ranked
 *     entries (the fraction is 0 when L == 1), sum_w = sum of w_p: per thread
 *     in CSR order, the threads in a fixed tree.
 * sums_out [HREC_RP_SUMS] (device f64): the sums over rows of auc,
 * reciprocal_rank, sum_w_pr, sum_w where each is defined (the last two: rows
 * with a ranked entry), then the four counts of those rows, then the ranked and
 * the unranked entries of all rows. Partials of 256 rows in the workspace,
 * added in a fixed order by a further launch, no floating-point atomics: equal
 * inputs give equal bits on every call.
 * A row's label entries are keyed and sorted HREC_RP_CHUNK at a time in LDS
 * and the score row is read once per chunk; nothing of size n_rows * n is
 * allocated. n < 2^31; n_rows == 0 returns HREC_OK and touches nothing.
 * Workspace: hrec_rank_positions_workspace_bytes(n_rows). */
#define HREC_RP_CHUNK 1024
#define HREC_RP_SUMS 10
size_t hrec_rank_positions_workspace_bytes(int64_t n_rows);
int hrec_rank_positions(int64_t n_rows, int64_t n, int source, const void* scores,
                        const float* tt_scores, int64_t ld, const double* als_fallback,
                        const double* minmax, const int32_t* row_wins, const int64_t* label_rows,
                        const int64_t* label_indptr, const int32_t* label_cols,
                        const double* label_weight, const int64_t* excl_rows,
                        const int64_t* excl_indptr, const int32_t* excl_cols, int32_t* out_rank,
                        double* out_row, int32_t* out_row_n, double* sums_out, void* workspace,
                        size_t workspace_bytes, void* stream);

/* What the served lists look like as a whole (additive to ABI 7): per list
 * its intra-list diversity, its unexpectedness against the user's history and
 * the means of per-item tables (novelty, popularity), and every item's
 * exposure over all lists.
 *
 * hrec_row_inv_norms: out[j] (f64, j < n) = 1 / sqrt(sum_c (double)v_jc^2) of
 * row j of vectors (f32 [n][ld], the first d columns), 0.0 when the sum is 0
 * or not finite: such an item is a zero vector below, whatever its components
 * are. 1 <= d <= 256, ld >= d, n < 2^31; n == 0 returns HREC_OK. One wave per
 * row: lane-strided f64 partials, then a fixed xor tree.
 *
 * hrec_list_quality: lists [n_rows][lists_ld] int64 holds candidate COLUMNS
 * (what every top-k here returns before the id gather: hrec_hybrid_lists'
 * out_idx, a hrec_topk_* / hrec_dot_topk* / hrec_als_score_topk* result), row
 * r's list in its first min(list_len[r], list_n) entries (list_len int32
 * [n_rows]; NULL: list_n). 0 <= list_n <= 1024, lists_ld >= list_n. vectors
 * f32 [n][ld] (1 <= d <= 256, ld >= d) and inv_norm f64 [n] (hrec_row_inv_norms
 * of them) describe the n candidates, 1 <= n < 2^31.
 * History (optional; a CSR shaped and addressed like the exclusion triple of
 * hrec_hybrid_lists): row r reads hist_cols[hist_indptr[q] .. hist_indptr[q +
 * 1]) with q = hist_rows[r]; q < 0, or all three pointers NULL: no history.
 * item_tables f64 [n_tab][n], 0 <= n_tab <= HREC_LQ_MAX_TABLES (NULL when 0).
 * An entry is valid when its position is below the row's length and its
 * column is in [0, n); every other entry (-1 included) is ignored everywhere
 * and never used as an index. The same holds for history columns (a history
 * column that appears twice counts twice). The entries of one list are
 * distinct items.
 * With the valid list entries a = 1..m, the valid history entries h = 1..g
 * and x_j = (double)v_j * inv_norm[j] componentwise (the zero vector where
 * inv_norm[j] == 0), all arithmetic f64 and unfused:
 *   S = sum_a x_a, Q = sum_a x_a.x_a, H = sum_h x_h;
 *   intraListDiversity = 1 - (S.S - Q) / (m (m - 1)): one minus the mean cosine
 *     over the pairs of distinct list entries; NaN when m < 2;
 *   unexpectedness = 1 - (S.H) / (m g): one minus the mean cosine between a
 *     list entry and a history entry; NaN when m == 0 or g == 0;
 *   per table t the mean of item_tables[t][col_a] over the entries where it
 *     is not NaN; NaN when there is none;
 *   exposure[col_a] += 1 (int64 [n], in and out) for every valid list entry,
 *     by integer atomics: the result does not depend on arrival order.
 * Outputs: per_row f64 [n_rows][2 + n_tab] = diversity, unexpectedness, the
 * table means; row_n int32 [n_rows][2 + n_tab] = m, g, then the counted
 * entries per table. sums_out f64 [2 * (2 + n_tab)] (device, IN AND OUT): the
 * call adds, per column, the sum over the rows where it is defined, then per
 * column the count of those rows; zero it before the first call of a series.
 * Lane l of a row's wave owns components l, l + 64, l + 128, l + 192 of S, H
 * and its part of Q; a row ends in three wave reductions (fixed xor trees).
 * Per-block partials in the workspace, added in a fixed order by a second
 * launch, no floating-point atomics: equal inputs give equal bits on every
 * call. n_rows == 0 returns HREC_OK and touches nothing.
 * Workspace: hrec_list_quality_workspace_bytes(n_rows). */
#define HREC_LQ_MAX_TABLES 4
int hrec_row_inv_norms(const float* vectors, int64_t n, int d, int64_t ld, double* out,
                       void* stream);
size_t hrec_list_quality_workspace_bytes(int64_t n_rows);
int hrec_list_quality(const int64_t* lists, int64_t lists_ld, int list_n, const int32_t* list_len,
                      int64_t n_rows, int64_t n, const float* vectors, int d, int64_t ld,
                      const double* inv_norm, const int64_t* hist_rows, const int64_t* hist_indptr,
                      const int32_t* hist_cols, const double* item_tables, int n_tab,
                      int64_t* exposure, double* per_row, int32_t* row_n, double* sums_out,
                      void* workspace, size_t workspace_bytes, void* stream);

/* Diversity-aware re-ranking of a candidate pool (additive to ABI 7): greedy
 * Maximal Marginal Relevance (Carbonell and Goldstein 1998), per list.
 *
 * hrec_mmr_rerank: pool [n_rows][pool_ld] int64 holds candidate COLUMNS, best
 * first (a top-k result before the id gather, as in hrec_list_quality), row
 * r's pool in its first min(pool_len[r], pool_n) entries (pool_len int32
 * [n_rows]; NULL: pool_n). scores [n_rows][scores_ld] holds the models'
 * ratings at the same positions, f32 (scores_f64 == 0) or f64 (1). vectors,
 * d, ld, inv_norm and n are hrec_list_quality's. 1 <= top_n <= pool_n <= 1024,
 * pool_ld >= pool_n, scores_ld >= pool_n, 1 <= d <= 256, ld >= d,
 * 0 <= lambda <= 1, 1 <= n < 2^31.
 * An entry is valid when its position is below the row's length and its
 * column is in [0, n); every other entry (-1 included) is never selected and
 * never used as an index. All arithmetic is f64 and unfused:
 *   x_p = (double)v_col(p) * inv_norm[col(p)] componentwise (the zero vector
 *     where inv_norm is 0, whatever the components are);
 *   lo, hi = the extremes of the finite scores of the row's valid entries;
 *   rel_p = (s_p - lo) / (hi - lo), 1.0 when hi == lo; a valid entry with a
 *     non-finite score takes no part in lo / hi and has value -inf at every
 *     step;
 *   at step t, with S the positions selected so far,
 *     value_p = lambda * rel_p - (1 - lambda) * max_{q in S} x_p . x_q
 *     (no clipping at 0; while S is empty, lambda * rel_p);
 *   step t selects the unselected valid position with the largest value,
 *     equal values: the smaller position.
 * Outputs: out_len[r] = min(top_n, valid entries of row r); out_pos int32
 * [n_rows][top_n] = the selected POSITIONS in the pool row, in selection
 * order, -1 past out_len; out_value f64 [n_rows][top_n] (optional) = the
 * selected entry's value at its step, NaN past out_len. So the first pick is
 * the best finite-scored valid entry, and lambda == 1 returns the valid
 * positions in pool order.
 * One block per list, one thread per pool position (up to four): a cosine is
 * a private chain of d terms in four partial sums (component c into sum c mod
 * 4, then (a0 + a1) + (a2 + a3)); rel, the running maximum and the selected
 * flag stay in registers. The arg-max is a fixed reduction over (value,
 * position): a wave xor tree, then the waves in order; no floating-point
 * atomics: equal inputs give equal bits on every call. The pool's rows are
 * staged in LDS once when pool_n * (d | 1) * 4 bytes fit 56 KiB, and re-read
 * from global memory at every step otherwise. No workspace.
 * n_rows == 0 returns HREC_OK and touches nothing. */
int hrec_mmr_rerank(const int64_t* pool, int64_t pool_ld, int pool_n, const int32_t* pool_len,
                    const void* scores, int scores_f64, int64_t scores_ld, int64_t n_rows,
                    int64_t n, const float* vectors, int d, int64_t ld, const double* inv_norm,
                    double lambda, int top_n, int32_t* out_pos, int32_t* out_len,
                    double* out_value, void* stream);

/* ALS predictions explained by the user's history (additive to ABI 7; Hu,
 * Koren and Volinsky 2008, section 5). A user row is the solution of its
 * normal equations, x = A^-1 b with b = sum_j beta_j y_j over the history, so
 * a prediction is a sum of one term per history entry:
 *   y_i . x = sum_j c_ij,   c_ij = beta_j * (y_i^T A^-1 y_j).
 *
 * hrec_als_explain: lists [n_rows][lists_ld] int64 holds candidate COLUMNS
 * (rows of item_factors; a top-k result before the id gather, as in
 * hrec_list_quality), row r's list in its first min(list_len[r], list_n)
 * entries (list_len int32 [n_rows]; NULL: list_n). 0 <= list_n <= 1024,
 * lists_ld >= list_n.
 * History: a CSR addressed like hrec_list_quality's, plus ratings: row r reads
 * hist_cols (int32 rows of item_factors) and hist_vals (f32 ratings) at
 * [hist_indptr[q], hist_indptr[q + 1]) with q = hist_rows[r]; q < 0: no
 * history. Several rows may name the same q (how a user with more than 1024
 * pairs is split). History columns outside [0, n_items) are an error of the
 * caller's (the half-sweeps' contract for CSR indices).
 * item_factors f32 [n_items][kp], kp = 16, 32 or 64, 1 <= k <= kp, padding
 * columns zero; reg_param >= 0; implicit 0 or 1; alpha >= 0; yty =
 * hrec_als_gramian of the same factors (required when implicit, ignored
 * otherwise); 1 <= top_m <= HREC_EXPLAIN_MAX_TOP.
 * Per row, with n history entries (duplicates stay separate terms):
 *   implicit == 0: A = sum_j y_j y_j^T + reg_param n I, beta_j = r_j; every
 *     entry is eligible (hrec_als_half_sweep's A and b);
 *   implicit == 1: c1_j = alpha |r_j|, A = yty + sum_j c1_j y_j y_j^T +
 *     reg_param n_pos I, beta_j = 1 + c1_j where r_j > 0 and 0 otherwise;
 *     the entries with r_j > 0 (n_pos of them) are eligible
 *     (hrec_als_half_sweep_implicit's A and b).
 * Sources are converted to f64 and accumulated in f64 on the matrix cores,
 * A = Ut^T D Ut once per row (the half-sweep's own pipeline). For each valid
 * list entry i: A w_i = y_i by two f64 substitutions, then per history entry
 * c_ij = beta_j * (w_i . y_j), the dot an f64 fma chain over the components in
 * ascending order.
 * Outputs (positions are POSITIONS WITHIN THE ROW'S HISTORY SEGMENT):
 *   out_total f64 [n_rows][list_n]: sum of c_ij over the eligible j — lane l
 *     of the row's wave adds entries l, l + 64, ... in order, then a fixed xor
 *     tree over the 64 partials;
 *   out_pos int32 / out_val f64 [n_rows][list_n][top_m]: the top_m largest
 *     c_ij of the eligible entries, descending, equal values: the earlier
 *     position first; past out_len, -1 and NaN;
 *   out_len int32 [n_rows][list_n] = min(top_m, eligible entries);
 *   out_row f32 [n_rows][kp] (optional, NULL skips it): the row's own solve
 *     A^-1 b, in the half-sweep's layout with its padding zeros — the bits
 *     the half-sweep stores for the same CSR row; zero for a row without
 *     history or (implicit) without a rating > 0.
 * A list entry past the row's length or outside [0, n_items) (-1 included) is
 * never used as an index and gets out_len 0, out_total NaN, positions -1 and
 * values NaN. So does every entry of a row without history, without an
 * eligible entry, or whose factorisation is unusable (a pivot that is not
 * positive and finite, or a non-finite x: reg_param = 0 with singular
 * equations).
 * One wave per row. No floating-point atomics and fixed orders throughout:
 * equal inputs give equal bits on every call. No workspace. n_rows == 0 or
 * list_n == 0 returns HREC_OK and touches nothing. */
#define HREC_EXPLAIN_MAX_TOP 32
int hrec_als_explain(const int64_t* lists, int64_t lists_ld, int list_n, const int32_t* list_len,
                     int64_t n_rows, const int64_t* hist_rows, const int64_t* hist_indptr,
                     const int32_t* hist_cols, const float* hist_vals, const float* item_factors,
                     int64_t n_items, int k, int kp, double reg_param, int implicit, double alpha,
                     const double* yty, int top_m, double* out_total, int32_t* out_pos,
                     double* out_val, int32_t* out_len, float* out_row, void* stream);

/* Cosine neighbours of rows of one matrix (additive to ABI 7): "more like
 * this" for item factors, user factors or tower vectors (the reference's
 * ALSModel._find_similar_items, src/als_model.py:93-104, keeps the top 3 with
 * sim > 0.5 and skips the item itself).
 *
 * hrec_cosine_topk: vectors f32 [n][ld], the first d columns (1 <= d <= 256,
 * ld >= d, 1 <= n < 2^31; the columns past d are never read); inv_norm f64 [n]
 * = hrec_row_inv_norms of them; query_rows int64 [n_q] names rows of the same
 * matrix (a row outside [0, n), -1 included, is an unknown query; repeats are
 * allowed; 0 <= n_q < 65536). 1 <= top_k <= 1024; skip_self 0 or 1; min_sim
 * f64 (-inf: no cut; NaN is an error); mode 0 auto, 1 exhaustive, 2 pruned.
 * The similarity, all f64 and unfused:
 *   dot(q, j) = the chain acc = acc + (double)v_q[c] * (double)v_j[c] for
 *     c = 0 .. d - 1 ascending, from 0.0 (the product of two f32 values is
 *     exact in f64, so a fused multiply-add gives the same bits);
 *   sim(q, j) = (dot * inv_norm[q]) * inv_norm[j]; +0.0 where inv_norm[q] == 0
 *     or inv_norm[j] == 0 (hrec_list_quality's zero-vector rule: a row with a
 *     zero or non-finite squared norm). Every sim is finite.
 * Per query b: the stable ranking of all columns j in [0, n) by sim, larger
 * first, equal sims -> the smaller j; with skip_self without column
 * query_rows[b]; cut to kk = min(top_k, n - skip_self) entries, then to the
 * prefix with sim > min_sim (strict).
 * Outputs: out_idx int64 / out_val f64 [n_q][top_k], out_len int32 [n_q]; past
 * out_len the entries are -1 and NaN; an unknown query has out_len 0.
 * Mode 1 writes the f64 sims of a sub-batch of queries to the workspace (the
 * query's own column as NaN) and ranks them with the f64 stable top-k. Mode 2
 * bounds every sim on the bf16 matrix cores from the prepared operand `items`
 * (hrec_cosine_items; may be NULL in mode 1, and in mode 0, which then takes
 * mode 1), runs the exact chain only for the rows a proven margin cannot rule
 * out and ranks those (csrc/cosine_topk.hip derives the margin). When a
 * query's kept list overflows, *overflow (device int, written by every call)
 * is set and the results of the call are incomplete: rerun it in mode 1.
 * Mode 0 takes mode 1 below a catalogue size fixed in the library (3072 rows,
 * from measurement) and where top_k * n is too large for the sample bound to
 * keep the lists within their capacity; like mode 2 it may set *overflow, and
 * one rerun in mode 1 always completes the call. Equal inputs give equal bits
 * on every call and in every mode (no floating-point atomics, fixed orders).
 * n_q == 0 returns HREC_OK and touches nothing.
 * Workspace: hrec_cosine_topk_workspace_bytes(n_q, n, top_k, d, mode).
 *
 * hrec_cosine_items: the operand of mode 2, once per matrix and reused by
 * every batch: bf16 rows [n][dk] of (float)((double)v_jc * inv_norm[j]), dk =
 * 32, 64, 128 or 256 columns (zero past d), a zero row where inv_norm is 0.
 * out: hrec_cosine_items_bytes(n, d) bytes, 256-B aligned.
 *
 * hrec_cosine_topk_counts (diagnostics, as hrec_als_score_topk_pruned_counts):
 * after a mode-2 call, out int32 [n_q] = the rows the filter kept per query,
 * read from that call's workspace (the same n_q, n, top_k and d); a count
 * above 4096 is a list that overflowed. */
size_t hrec_cosine_items_bytes(int64_t n, int d);
int hrec_cosine_items(const float* vectors, int64_t n, int d, int64_t ld, const double* inv_norm,
                      void* out, void* stream);
size_t hrec_cosine_topk_workspace_bytes(int n_q, int64_t n, int top_k, int d, int mode);
int hrec_cosine_topk(const float* vectors, int64_t n, int d, int64_t ld, const double* inv_norm,
                     const int64_t* query_rows, int n_q, int top_k, int skip_self, double min_sim,
                     int mode, const void* items, int64_t* out_idx, double* out_val,
                     int32_t* out_len, int* overflow, void* workspace, size_t workspace_bytes,
                     void* stream);
int hrec_cosine_topk_counts(const void* workspace, int n_q, int64_t n, int top_k, int d,
                            int32_t* out, void* stream);

/* ------------------------------------------------------ cold-start sim --
 * ALSModel._find_similar_items (src/als_model.py:93-104): out[q*n_items+j] =
 * cosine(feats[query_rows[q]], feats[j]) with sklearn's normalise-then-dot
 * (a norm below 10 * DBL_EPSILON, zero included, -> 1: such a row is not
 * scaled up); the query's own entry is -inf (the reference skips it).
 * feats: [n_items, dim] f64 row-major in item_features dict order. */
int hrec_cosine_sim(const double* feats, int64_t n_items, int dim,
                    const int64_t* query_rows, int64_t n_query, double* out,
                    void* stream);

/* The cold-start fallback of EVERY item, once per model (src/als_model.py
 * :78-86 + _find_similar_items :93-104; the value depends on the item only):
 * out_mean[i] = the mean 'rating' (ratings[j], f64) of the <= 3 items j != i
 * most similar to i (hrec_cosine_sim's values, ranked larger first, ties ->
 * smaller j) with similarity > 0.5, as np.mean sums them ((r0 + r1) + r2) /
 * count; out_count[i] = how many (0: the caller's global mean; out_mean 0);
 * out_idx (optional, [n_items][3] int32, -1 padded) = those j in rank order.
 * feats [n_items][dim] f64 row-major, dim <= 16, n_items < 2^31. One pass of
 * n_items^2 similarities, no similarity matrix in memory.
 * Workspace: hrec_cold_fallback_workspace_bytes(n_items, dim). */
size_t hrec_cold_fallback_workspace_bytes(int64_t n_items, int dim);
int hrec_cold_fallback(const double* feats, const double* ratings, int64_t n_items, int dim,
                       double* out_mean, int32_t* out_count, int32_t* out_idx, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------ two-tower --
 * Keras graph of src/two_tower_model.py:38-89 (embedding_size d):
 *   user_vec = LN_u(E_user[u]);  h = relu(numeric @ W1 + b1)  [Dense(16)]
 *   z = [E_item[i] | E_man[m] (8) | E_cat[c] (8) | h (16)]    (d+32)
 *   item_vec = LN_i(z @ W2 + b2) [Dense(d)];  score = <user_vec, item_vec>
 * LayerNormalization: epsilon 1e-3, biased variance, y = xhat*gamma + beta.
 * All tensors f32 row-major on the device; ids int32 (< 2^24, see D11). */
typedef struct hrec_tt_params {
  int32_t d;
  int32_t reserved;
  float* user_emb;      /* [n_users, d]    */
  float* item_emb;      /* [n_items, d]    */
  float* man_emb;       /* [n_man, 8]      */
  float* cat_emb;       /* [n_cat, 8]      */
  float* w1;            /* [2, 16]         */
  float* b1;            /* [16]            */
  float* w2;            /* [d + 32, d]     */
  float* b2;            /* [d]             */
  float* ln_user_gamma; /* [d] */
  float* ln_user_beta;  /* [d] */
  float* ln_item_gamma; /* [d] */
  float* ln_item_beta;  /* [d] */
} hrec_tt_params;

/* Item tower over n candidate rows (the per-candidate graph evaluated by
 * model.predict at src/two_tower_model.py:145). */
int hrec_tt_item_forward(const hrec_tt_params* params, const int32_t* item,
                         const int32_t* manufacturer, const int32_t* category,
                         const float* numeric /* [n,2] */, int64_t n,
                         float* item_vec /* [n,d] */, void* stream);
/* User tower for n users. */
int hrec_tt_user_forward(const hrec_tt_params* params, const int32_t* user, int64_t n,
                         float* user_vec /* [n,d] */, void* stream);
/* Dot(axes=1) of every user row with every item row: out[b*n_items + j]
 * (f32). Every two-tower score in libhrec (this call at any n_users,
 * hrec_tt_pair_score, hrec_dot_scores / hrec_dot_topk on f32 operands, the
 * exact hybrid) is one fmaf chain from zero in one k order, so a score's bits
 * do not depend on the batch: d in {32, 64, 128, 256}: steps of 16, inside a
 * step k = 16 s + 4 g + e with g fastest (the v_mfma_f32_16x16x4_f32 tiles);
 * any other d: k = 0 .. d-1. */
int hrec_tt_score(const float* user_vec, int n_users, const float* item_vec,
                  int64_t n_items, int d, float* out, void* stream);

/* The item tower's inputs of one predict_for_user call from the candidate
 * frame's raw columns (src/two_tower_model.py:136-146): item / manufacturer /
 * category ids (int64) -> int32 (each in [0, its table) and below 2^24, where
 * Keras' float32 Input round trip is the identity), numeric [n,2] f32 =
 * (price, rating) * scale + min in f64 (MinMaxScaler.transform), rounded once.
 * scale / min_: HOST arrays of 2 doubles (the fitted scaler's scale_ / min_).
 * *flags (device int32, written by the call): bit 1 an id outside those
 * bounds, bit 2 an infinite numeric input, bit 4 a repeated item id — the
 * outputs are then unusable and the caller takes the host path (which raises
 * the reference's error where it raises). Replaces the host-side _ids casts,
 * scaler.transform and the candidate-uniqueness pass of the hybrid's array
 * path (src/hybrid_system.py:95-116). */
size_t hrec_tt_item_inputs_workspace_bytes(int64_t n_item_table);
int hrec_tt_item_inputs(const int64_t* item, const int64_t* manufacturer, const int64_t* category,
                        const double* price, const double* rating, int64_t n, int64_t n_item_table,
                        int64_t n_man_table, int64_t n_cat_table, const double* scale, const double* min_,
                        int32_t* item_out, int32_t* man_out, int32_t* cat_out, float* numeric_out,
                        int32_t* flags, void* workspace, size_t workspace_bytes, void* stream);

/* Row-wise dot: out[r] = <user_vec[r], item_vec[r]> (n rows of d), in
 * hrec_tt_score's order (the same bits for the same pair). */
int hrec_tt_pair_score(const float* user_vec, const float* item_vec, int64_t n, int d,
                       float* out, void* stream);

/* Two-tower scores of a pair list, and the regression sums over them
 * (csrc/tt_pairs.hip; the two-tower counterpart of hrec_als_predict_pairs /
 * hrec_als_pair_metrics).
 * hrec_tt_predict_pairs: out[p] = <user_vec[user_rows[p]],
 * item_vec[item_rows[p]]> for p < n. user_vec [n_user_rows, d] and item_vec
 * [n_item_rows, d] are dense f32 with row stride d (what hrec_tt_user_forward
 * / hrec_tt_item_forward write), 1 <= d <= 256, each matrix aligned to 16 B
 * when d % 4 == 0, to 8 B when d % 2 == 0, to 4 B otherwise. The chain is
 * hrec_tt_score's (an fmaf chain from zero in its k order for this d), so a
 * pair has the bits hrec_tt_pair_score and hrec_tt_score give it. A row index
 * outside [0, n_rows) on either side gives a quiet NaN and is never turned
 * into an address. n == 0 is a no-op.
 * hrec_tt_pair_metrics: the same predictions (stored when pred_out is not
 * null) against labels (f64 [n]); sums_out[HREC_PAIR_SUMS] (device f64) has
 * the HREC_PAIR_* layout and meaning of hrec_als_pair_metrics, with p^ =
 * (double)prediction and e = y - p^. Pairs with a NaN prediction (a bad row
 * index, a NaN in either vector) count in HREC_PAIR_N_NAN and enter no sum.
 * No floating-point atomics: per-block partials in the workspace (the block
 * count depends on n alone), added in a fixed order by a second launch, so
 * equal inputs give equal bits on every call; n == 0 writes zeros.
 * Workspace: hrec_tt_pair_metrics_workspace_bytes(n). */
int hrec_tt_predict_pairs(const float* user_vec, int64_t n_user_rows,
                          const float* item_vec, int64_t n_item_rows, int d,
                          const int64_t* user_rows, const int64_t* item_rows, int64_t n,
                          float* out, void* stream);
size_t hrec_tt_pair_metrics_workspace_bytes(int64_t n);
int hrec_tt_pair_metrics(const float* user_vec, int64_t n_user_rows,
                         const float* item_vec, int64_t n_item_rows, int d,
                         const int64_t* user_rows, const int64_t* item_rows, int64_t n,
                         const double* labels, float* pred_out, double* sums_out,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Fold users into the two-tower model (csrc/tt_fold_in.hip): row u of emb
 * [n_rows, d] (f32, row stride d; in: the start rows, out: the fitted rows) is
 * fitted to its own history - the entries indptr[u] .. indptr[u + 1] of
 * (item_rows, ratings), int64 indptr [n_rows + 1] - with every other variable
 * frozen: what model.fit does to that user-embedding row when the user's whole
 * history is one batch per step. ln_gamma / ln_beta [d]: the user tower's
 * LayerNormalization; item_vec [n_items, d]: hrec_tt_item_forward's output.
 * The usable history is the entries with 0 <= item_rows[j] < n_items (n of
 * them; duplicates stay separate terms); the others are skipped and never
 * turned into an address. For t = 1 .. steps, all in f32:
 *   xh = (e - mean(e)) rsqrt(var(e) + 1e-3) (biased variance), u = xh gamma + beta
 *   err_j = <u, item_vec[item_rows[j]]> - ratings[j], usable entries in CSR order
 *   du = (2 / n) sum_j err_j item_vec[item_rows[j]],  dxh = du gamma
 *   g = rstd (dxh - mean(dxh) - xh mean(dxh xh))
 *   m = m beta1 + g one_minus_beta1;  v = v beta2 + g^2 one_minus_beta2
 *   e -= step_lr[t - 1] m / (sqrt(v) + epsilon)            (m = v = 0 before t = 1)
 * i.e. Keras' sparse Adam for a row touched at every step; step_lr (device f32
 * [steps]) holds lr sqrt(1 - beta2^t) / (1 - beta1^t) per step.
 * out_loss (optional, [n_rows][2]): mean_j err_j^2 at the start row and after
 * the last step. n == 0 leaves the row as it was and writes NaN, NaN; steps ==
 * 0 leaves every row as it was and writes the same loss twice. 1 <= d <= 256;
 * emb and item_vec aligned as hrec_tt_predict_pairs asks for d. One wave per
 * row, no atomics, every sum in a fixed order: equal inputs give equal bits.
 * Rows of emb beyond n_rows are not touched; n_rows == 0 is a no-op. The
 * caller guarantees a well-formed CSR: indptr non-decreasing, 0 <= indptr[0],
 * indptr[n_rows] <= the length of item_rows and ratings (device data, not
 * checked here). */
int hrec_tt_fold_in_users(float* emb, int64_t n_rows, int d,
                          const float* ln_gamma, const float* ln_beta,
                          const float* item_vec, int64_t n_items,
                          const int64_t* indptr, const int64_t* item_rows, const float* ratings,
                          int steps, const float* step_lr,
                          float beta1, float one_minus_beta1, float beta2, float one_minus_beta2,
                          float epsilon, float* out_loss, void* stream);

/* One minibatch of model.fit (src/two_tower_model.py:111): forward, MSE
 * loss, backward. grad_dense receives hrec_tt_grad_len(d) floats:
 * dW2[(d+32)*d] | db2[d] | dgamma_i[d] | dbeta_i[d] | dgamma_u[d] | dbeta_u[d]
 * | dW1[32] | db1[16] | sum_sq_err[1] | sum_abs_err[1]  (loss = sum_sq_err/batch).
 * g_user/g_item [batch,d], g_man/g_cat [batch,8]: per-sample embedding-row
 * gradients (IndexedSlices values, duplicates not yet summed). */
size_t hrec_tt_train_workspace_bytes(int d, int64_t batch);
size_t hrec_tt_grad_len(int d);
int hrec_tt_forward_backward(const hrec_tt_params* params, const int32_t* user,
                             const int32_t* item, const int32_t* manufacturer,
                             const int32_t* category, const float* numeric,
                             const float* y, int64_t batch, float* grad_dense,
                             float* g_user, float* g_item, float* g_man, float* g_cat,
                             void* workspace, size_t workspace_bytes, void* stream);

/* TF 2.8 ResourceApplyAdam (dense variables): m += (g-m)(1-b1);
 * v += (g^2-v)(1-b2); var -= m*alpha/(sqrt(v)+eps). alpha (host, f32) =
 * lr*sqrt(1-b2^t)/(1-b1^t). */
int hrec_adam_dense(float* var, float* m, float* v, const float* grad, int64_t n,
                    float alpha, float beta1, float beta2, float epsilon, void* stream);
/* Keras OptimizerV2 Adam._resource_apply_sparse on an embedding table:
 * duplicate indices summed in sample order (tf.unique + segment sum), then
 * m = m*b1 (whole table), m[idx] += g*(1-b1); v likewise with g^2; var -=
 * lr*m/(sqrt(v)+eps) over the WHOLE table. mark: int32[n_rows] all -1 on
 * entry (restored on exit); gsum: [batch, dim] scratch. */
int hrec_adam_sparse(float* var, float* m, float* v, int64_t n_rows, int dim,
                     const int32_t* indices, const float* grad_rows, int batch,
                     int32_t* mark, float* gsum, float lr, float beta1,
                     float one_minus_beta1, float beta2, float one_minus_beta2,
                     float epsilon, void* stream);

/* hrec_adam_sparse over several tables in one set of launches (the four
 * embedding tables of one Keras train step, src/two_tower_model.py:85,111):
 * per table exactly hrec_adam_sparse's arithmetic; 3 launches in total
 * instead of 3 per table. At most HREC_MAX_SPARSE_TABLES tables. */
#define HREC_MAX_SPARSE_TABLES 8
typedef struct hrec_sparse_table {
  float* var;
  float* m;
  float* v;
  int64_t n_rows;
  int32_t dim;
  int32_t batch;
  const int32_t* indices;
  const float* grad_rows;
  int32_t* mark;
  float* gsum;
} hrec_sparse_table;

int hrec_adam_sparse_tables(const hrec_sparse_table* tables, int n_tables, float lr,
                            float beta1, float one_minus_beta1, float beta2,
                            float one_minus_beta2, float epsilon, void* stream);

/* hrec_adam_sparse_tables in phases, for a two-stream train step: the
 * whole-table sweep of the rows the batch does NOT touch (phase 1, nearly all
 * of the step's HBM bytes) runs on a second stream beside the batch's
 * forward / backward, which read only touched rows; phase 2 then sums the
 * batch's gradients and steps the touched rows. Phases 0..3 in order give
 * bit for bit the rows of hrec_adam_sparse_tables (same Keras IndexedSlices
 * Adam, src/two_tower_model.py:111 via model.fit). Phase 1 may overlap phase
 * 2, never phase 0 or 3. Needs dim % 4 == 0 and 16-B aligned var/m/v; gsum
 * is not used, grad_rows only by phase 2. */
#define HREC_SPARSE_MARK 0
#define HREC_SPARSE_SWEEP_UNTOUCHED 1
#define HREC_SPARSE_TOUCHED 2
#define HREC_SPARSE_UNMARK 3
int hrec_adam_sparse_tables_phase(const hrec_sparse_table* tables, int n_tables, int phase,
                                  float lr, float beta1, float one_minus_beta1, float beta2,
                                  float one_minus_beta2, float epsilon, void* stream);

/* ---------------------------------------------------------------------
 * Matrix-core dot-product scoring + fused top-k (csrc/dot_topk.hip).
 * Replaces Keras Dot(axes=1) over every candidate in model.predict
 * (src/two_tower_model.py:80, :136-146) and the ranking after it
 * (sorted(..., reverse=True)[:k], src/hybrid_system.py:108), at BASELINE
 * configs c4 (d = 128, 50M candidates) and c5 (bf16, d = 256).
 * Operands: row-major [n, dk] with dk in {32, 64, 128, 256} (the model's d
 * zero-padded), 16-B aligned; dtype 0 = f32 (exact f32 fma chains on
 * v_mfma_f32_16x16x4_f32, k order permuted), 1 = bf16 bit patterns
 * (v_mfma_f32_16x16x32_bf16, f32 accumulation). n_items < 2^31. */
int hrec_f32_to_bf16(const float* in, int64_t n, uint16_t* out, void* stream);
/* out[b*ld_out + j] = <U[b], V[j]> for b < n_users, j < n_items.
 * Summation order and batch size: f32 calls of 1-4 users run the streaming
 * GEMV kernel, larger batches the matrix-core tiles; both issue the same
 * v_mfma_f32_16x16x4_f32 sequence per score (k order 16 ks + 4 g + e), so a
 * user's scores have the same bits at every batch size. bf16 calls always use
 * the matrix-core tiles. The same holds for hrec_dot_topk. */
int hrec_dot_scores(const void* user_vec, int n_users, const void* item_vec, int64_t n_items, int dk,
                    int dtype, float* out, int64_t ld_out, void* stream);
size_t hrec_dot_topk_workspace_bytes(int n_users, int64_t n_items, int top_k);
/* Stable top-k (larger first, ties -> smaller item index) of every user's
 * scores over items [0, n_items), without writing the score matrix: the
 * k-th best of a strided item sample (or thr_in[b] when thr_in != NULL) is a
 * lower bound of the k-th best; a fused score + filter pass appends the
 * survivors to a per-user list, ranked by an exact stable top-k. out_idx
 * gets idx_offset added (item shards). *overflow != 0 when a user had more
 * survivors than the list holds — then rerun with thr_in = out_val[:, k-1]
 * (the k-th best survivor is a higher valid bound). n_users < 65536. */
int hrec_dot_topk(const void* user_vec, int n_users, const void* item_vec, int64_t n_items, int dk,
                  int dtype, int top_k, const float* thr_in, int64_t idx_offset, int64_t* out_idx,
                  float* out_val, int* overflow, void* workspace, size_t workspace_bytes,
                  void* stream);
/* hrec_dot_topk over the items a query has not seen: the same scores (the
 * bits hrec_dot_scores gives each pair), the same stable ranking, with the
 * items of the query's exclusion set deleted from it, cut to kk = min(top_k,
 * n_items). Additive to ABI 7.
 *
 * The set of query b is excl_cols[excl_indptr[r] .. excl_indptr[r + 1]) with
 * r = excl_rows[b] (a negative r: the empty set) — hrec_mask_rows_f32's
 * convention. Columns are LOCAL item indices in [0, n_items), before
 * idx_offset is added; ascending; duplicates count once; a column outside the
 * range is ignored and never used as an index. out_len[b] (int32, device) =
 * min(kk, n_items - distinct in-range excluded columns of b), computed from
 * the exclusion row; the entries of out_idx / out_val at positions >=
 * out_len[b] are unspecified.
 * Catalogues hrec_dot_topk scores in full (n_items <= 16384, no thr_in): the
 * excluded scores become NaN (ranked last) before the exact top-k. Otherwise
 * the bound is the kk-th best of the strided sample's items that stay (the
 * sample columns of excluded items are set to -inf first; a query with fewer
 * than kk of them left gets -inf and admits every score), the three filter
 * kernels run unchanged, and the excluded candidates leave the lists (NaN
 * scores) before the final top-k. *overflow as hrec_dot_topk sets it: some
 * query had more survivors than its list holds, excluded ones included.
 * thr_in keeps its meaning (a NaN entry admits every score); after an
 * overflowed round out_val[:, kk - 1] is again a valid higher bound — NaN,
 * which admits everything, when fewer than kk non-excluded entries sat in the
 * truncated list — so the refinement round of hrec_dot_topk carries over. A
 * caller out of rounds falls back to hrec_dot_scores + hrec_mask_rows_f32
 * (fill NaN) + hrec_topk_f32. Operands, limits and workspace size are
 * hrec_dot_topk's. */
size_t hrec_dot_topk_excluding_workspace_bytes(int n_users, int64_t n_items, int top_k);
int hrec_dot_topk_excluding(const void* user_vec, int n_users, const void* item_vec, int64_t n_items,
                            int dk, int dtype, int top_k, const float* thr_in, int64_t idx_offset,
                            const int64_t* excl_rows, const int64_t* excl_indptr, const int32_t* excl_cols,
                            int64_t* out_idx, float* out_val, int32_t* out_len, int* overflow,
                            void* workspace, size_t workspace_bytes, void* stream);
/* The survivor filter of hrec_dot_topk / the pruned hybrid alone: append
 * (score, j) of every item j with <U[b], V[j]> >= thr[b * thr_stride + (thr_per
 * ? j / thr_per : 0)] to user b's list (cand_val / cand_idx [n_users, cap]; a
 * NaN bound admits every score, a +inf bound none — a dead user or group,
 * skipped; hrec_dot_topk's own filter instead admits scores >= +inf for a
 * +inf bound; list order unspecified). cand_n[b], zeroed by
 * the caller, ends as the user's survivor count, or > cap when the list
 * overflowed (the list then holds an arbitrary subset). bf16 operands, or f32
 * at dk <= 128. */
int hrec_dot_filter(const void* user_vec, int n_users, const void* item_vec, int64_t n_items, int dk,
                    int dtype, const float* thr, int thr_stride, int64_t thr_per, int cap, float* cand_val,
                    int64_t* cand_idx, int* cand_n, void* stream);

/* ---------------------------------------------------------------------
 * Both score matrices of the bf16 hybrid in one launch (csrc/hybrid_scores.hip,
 * BASELINE config c5): the scores get_hybrid_recommendations ranks per user
 * (ALS transform + Keras Dot over every candidate, src/hybrid_system.py:95-116)
 * and the per-model MinMaxScaler extremes it fits (src/hybrid_system.py:57-75).
 * User rows are f32 (ALS: als_users[als_rows[b] * als_ld + c], als_rows may
 * be NULL for row b; a row outside [0, n_als_rows) — an unknown user — gives
 * a NaN score row, as hrec_als_score does for row -1, whose min / max are
 * +inf / -inf; two-tower: tt_users[b * tt_ld + c]), converted to bf16
 * (round to nearest even) for columns c < width and zero up to dk; item
 * operands are bf16 [n_items, dk], dk in {64, 128, 256}. Writes
 * als_out / tt_out [n_users, ld_out] f32 (bit-identical to hrec_dot_scores on
 * hrec_f32_to_bf16 operands) and als_mm / tt_mm [2, n_users] f32 =
 * hrec_rows_minmax_f32 of those rows. */
size_t hrec_hybrid_scores_workspace_bytes(int n_users, int64_t n_items);
int hrec_hybrid_scores(const float* als_users, int64_t als_ld, const int64_t* als_rows,
                       int64_t n_als_rows, int als_width,
                       const float* tt_users, int64_t tt_ld, int tt_width, int n_users,
                       const void* als_items, const void* tt_items, int64_t n_items, int dk,
                       float* als_out, float* tt_out, int64_t ld_out, float* als_mm, float* tt_mm,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------
 * Pruned bf16 hybrid top-k (csrc/hybrid_prune.hip, BASELINE config c5):
 * get_hybrid_recommendations for a batch of users over an item shard
 * (src/hybrid_system.py:57-75, :108) without writing either score matrix.
 * Same arguments as hrec_hybrid_scores for the users / items; results bit for
 * bit those of hrec_hybrid_scores + hrec_fuse_rows_topk.
 * Phase 1 (hrec_hybrid_prune_minmax): per-user [min | max] of both score rows
 *   into als_mm / tt_mm ([2, n_users] f32, the hrec_rows_minmax_f32 layout)
 *   and, in the workspace, each item group's maximum slice. With the items
 *   sharded, all-reduce the mins (MIN) and maxes (MAX) across shards before
 *   phase 2.
 * Phase 2 (hrec_hybrid_prune_topk): with the (global) min / max: a lower
 *   bound of each user's k-th best fused score from the group maxima, the
 *   heavier-weighted model's scores filtered against it, the survivors' other
 *   score and fused score, the stable top-k (ties -> smaller item; ids +
 *   idx_offset). Lists that overflow, users with non-finite scores or fewer
 *   survivors than k take the exact unfused path, gated on the device (no host
 *   round trip; hrec_hybrid_prune_fallback_taken copies that flag).
 * top_k in [1, 8]; the workspace (hrec_hybrid_prune_workspace_bytes, the same
 * dk and top_k) carries phase 1's state into phase 2: per item group G =
 * ceil(n_items / group) the group partials and arg-slices (24 B per user and
 * group), both bf16 user operands (4 dk B per user), the per-group bounds
 * (4 B per user and group) and each user's survivor list of 8192 entries
 * (96 KiB per user, whatever n_items is; the exact fallback runs inside the
 * survivor kernel and needs no score matrices). About 100 KiB per user at
 * c5: 25 MB for 256 users. n_users < 65536. */
size_t hrec_hybrid_prune_workspace_bytes(int n_users, int64_t n_items, int dk, int top_k);
int hrec_hybrid_prune_minmax(const float* als_users, int64_t als_ld, const int64_t* als_rows,
                             int64_t n_als_rows, int als_width, const float* tt_users, int64_t tt_ld,
                             int tt_width, int n_users, const void* als_items, const void* tt_items,
                             int64_t n_items, int dk, float* als_mm, float* tt_mm, void* workspace,
                             size_t workspace_bytes, void* stream);
int hrec_hybrid_prune_topk(const float* als_users, int64_t als_ld, const int64_t* als_rows,
                           int64_t n_als_rows, int als_width, const float* tt_users, int64_t tt_ld,
                           int tt_width, int n_users, const void* als_items, const void* tt_items,
                           int64_t n_items, int dk, const float* als_mm, const float* tt_mm, int als_wins,
                           int top_k, int64_t idx_offset, int64_t* out_idx, double* out_val,
                           void* workspace, size_t workspace_bytes, void* stream);
int hrec_hybrid_prune_fallback_taken(const void* workspace, int n_users, int64_t n_items, int dk,
                                     int top_k, int* out, void* stream);
/* Both phases for ONE item shard (no cross-shard min / max to combine): the
 * same results as hrec_hybrid_prune_minmax + hrec_hybrid_prune_topk (als_mm /
 * tt_mm are outputs here, [2, n_users] f32) with one launch fewer (the bound
 * kernel reduces the extremes). Same workspace. */
int hrec_hybrid_prune_local(const float* als_users, int64_t als_ld, const int64_t* als_rows, int64_t n_als_rows,
                            int als_width, const float* tt_users, int64_t tt_ld, int tt_width, int n_users,
                            const void* als_items, const void* tt_items, int64_t n_items, int dk, int als_wins,
                            int top_k, int64_t idx_offset, float* als_mm, float* tt_mm, int64_t* out_idx,
                            double* out_val, void* workspace, size_t workspace_bytes, void* stream);
/* Diagnostics of the last phase 2: the survivors of the heavy-model filter per
 * user (out: n_users int32, device). */
int hrec_hybrid_prune_survivors(const void* workspace, int n_users, int64_t n_items, int dk, int top_k,
                                int32_t* out, void* stream);

/* ---------------------------------------------------------------------
 * Exact hybrid top-k without score matrices (csrc/hybrid_exact.hip, BASELINE
 * config c2): get_hybrid_recommendations for a batch of users over an item
 * shard (src/hybrid_system.py:57-75, :95-116) with the reference's numerics —
 * the JVM-exact ALS dot (Spark ALSModel.transform, src/als_model.py:75) and
 * the f32 Keras Dot (src/two_tower_model.py:80) in hrec_dot_scores' MFMA k
 * order — bit for bit the result of hrec_als_score + hrec_tt_score (any
 * n_users >= 1) + hrec_rows_minmax_f32 + hrec_fuse_rows_topk, without writing either
 * [n_users, n_items] score matrix: both models are approximated on the bf16
 * matrix cores with a rigorous error bound, and only the item groups the
 * bound cannot rule out (a model's extremes; the fused top-k) are rescored
 * with the exact chains.
 *   als_users[als_rows[b] * als_ld + c], c < als_width (a row outside
 *     [0, n_als_rows) is an unknown user: NaN ALS scores);
 *   tt_users[b * tt_ld + c], c < tt_width in {32, 64, 128};
 *   als_items_t: the shard's ALS item factors transposed (item j, column c
 *     at als_items_t[c * als_items_ld + j]: hrec_als_score's layout);
 *   tt_items: the shard's two-tower item vectors, row-major (row stride a
 *     multiple of 4, 16-B aligned), tt_items_t the same transposed;
 *   prepared: hrec_hybrid_exact_prepare's split-bf16 operands + norm bounds
 *     of the same items (hrec_hybrid_exact_items_bytes, once per shard);
 *   dk in {64, 128} >= both widths. n_users < 65536. */
typedef struct hrec_hybrid_batch {
  const float* als_users;
  const int64_t* als_rows;
  const float* tt_users;
  const float* als_items_t;
  const float* tt_items;
  const float* tt_items_t;
  const void* prepared;
  int64_t als_ld;
  int64_t n_als_rows;
  int64_t tt_ld;
  int64_t als_items_ld;
  int64_t tt_items_ld;
  int64_t tt_items_t_ld;
  int64_t n_items;
  int32_t als_width;
  int32_t tt_width;
  int32_t n_users;
  int32_t dk;
} hrec_hybrid_batch;
size_t hrec_hybrid_exact_items_bytes(int64_t n_items, int dk);
int hrec_hybrid_exact_prepare(const float* als_items_t, int64_t als_ld, int als_width, const float* tt_items,
                              int64_t tt_ld, int tt_width, int64_t n_items, int dk, void* out, void* stream);
/* Workspace (the same dk) carrying phase 1 into phase 2: 16 B per user and
 * 32-item group + the bf16 user operands — 12.8 MB for 256 users x 100k items. */
size_t hrec_hybrid_exact_workspace_bytes(int n_users, int64_t n_items, int dk);
/* Phase 1 + the exact extremes: als_mm / tt_mm [2, n_users] f32 (the
 * hrec_rows_minmax_f32 layout). All-reduce them across item shards, then: */
int hrec_hybrid_exact_minmax(const hrec_hybrid_batch* batch, float* als_mm, float* tt_mm, void* workspace,
                             size_t workspace_bytes, void* stream);
/* the stable top-k (ties -> smaller item; ids + idx_offset) with the (global)
 * extremes; top_k in [1, 8]. */
int hrec_hybrid_exact_topk(const hrec_hybrid_batch* batch, const float* als_mm, const float* tt_mm, int als_wins,
                           int top_k, int64_t idx_offset, int64_t* out_idx, double* out_val, void* workspace,
                           size_t workspace_bytes, void* stream);
/* Both for ONE shard (als_mm / tt_mm are outputs): 3 launches. */
int hrec_hybrid_exact_local(const hrec_hybrid_batch* batch, int als_wins, int top_k, int64_t idx_offset,
                            float* als_mm, float* tt_mm, int64_t* out_idx, double* out_val, void* workspace,
                            size_t workspace_bytes, void* stream);
/* Diagnostics of the last call: out[b] = item groups rescored for user b's
 * exact extremes, out[n_users + b] = for its top-k, out[2 n_users] = 1 when
 * some user rescored every group (int32, device). */
int hrec_hybrid_exact_counts(const void* workspace, int n_users, int64_t n_items, int dk, int32_t* out,
                             void* stream);

/* ---------------------------------------------------------------------
 * Multi-GPU exchange steps (csrc/comm.hip) for hosts without
 * torch.distributed: one process per GPU, RCCL over xGMI (bound with dlopen
 * at hrec_comm_init; a process that already loaded librccl.so.1 — PyTorch —
 * shares that copy). Rank 0 calls hrec_comm_get_unique_id and hands the 128
 * bytes to every rank (the host's own channel); every rank then calls
 * hrec_comm_init (collective). HREC_E_UNSUPPORTED when RCCL is absent.
 *   C1: hrec_allgather of a rank's factor rows after a half-sweep (recv =
 *       world x count elements, rank-major: the replicated matrix);
 *   C2: hrec_allreduce_minmax — mm is [n_rows][2][n_users] f32 (each model's
 *       [min; max] rows, the hrec_rows_minmax_f32 layout, models consecutive),
 *       replaced in place by the minima / maxima over all ranks (one MIN
 *       all-reduce with the maxima negated);
 *   C3: hrec_allgather (dtype 4 = bytes) of the per-shard top-k candidates. */
int hrec_comm_get_unique_id(uint8_t* id_out /* 128 bytes */);
int hrec_comm_init(int rank, int world, const uint8_t* id /* 128 bytes */, void** comm_out);
int hrec_comm_destroy(void* comm);
/* dtype: 0 f32, 1 f64, 2 i32, 3 i64, 4 u8; count = elements per rank. */
int hrec_allgather(void* comm, const void* send, void* recv, size_t count, int dtype, void* stream);
int hrec_allreduce_minmax(void* comm, float* mm, int n_rows, int64_t n_users, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* HREC_H */
