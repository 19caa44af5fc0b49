/*
 * tmf.h - C ABI of libtmf.so, the MI355X (gfx950) engine behind
 * teamoflow.mf.MatrixFactorization.fit / predict / recall_at_k / retrieve_user_recs.
 *
 * The reference (GitHubOfAndrew/TeAMOFlow v0.0.2) has no FFI of its own: its hot path is a
 * sequence of TensorFlow eager ops issued from src/teamoflow/mf/matrix_factorization.py.  Each
 * entry point below replaces one group of those call sites (cited per function, paths relative to
 * the reference's src/teamoflow/mf/).  The Python host (teamoflow_amd/_lib.py) binds them with
 * ctypes; INTEGRATION.md shows the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a BORROWED DEVICE pointer (owned by the caller, e.g. a torch tensor);
 *     nothing is allocated, freed or synchronised inside the library;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it and the call returns
 *     immediately (graph-capture safe);
 *   - return value 0 = success, negative = TMF_E_* below; tmf_last_error() gives a thread-local
 *     message for the last failing call on this thread;
 *   - factor tables are fp32 row-major [rows, ld] with ld = tmf_padded_ld(n_components); the
 *     columns [n_components, ld) are zero and stay zero;
 *   - ids are int32, offsets into interaction / sample lists are int64.
 */
#ifndef TMF_H
#define TMF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMF_VERSION 203 /* 0.2.3: the balanced row-stationary item pass tmf_wsum_rows5; the 72-byte tmf_slice_lists carries `flags`: n_items counts only with TMF_SLICE_N_ITEMS_STATED */

#define TMF_OK 0
#define TMF_E_INVALID (-1)   /* bad argument (null pointer, unsupported rank, size mismatch) */
#define TMF_E_LAUNCH (-2)    /* hipLaunch / runtime error, text in tmf_last_error() */
#define TMF_E_UNSUPPORTED (-3)

/* epilogue selector of the row passes */
#define TMF_EPI_ADAM 0 /* out[row] = fresh-Adam(old[row], g[row])  (matrix_factorization.py:176) */
#define TMF_EPI_GRAD 1 /* out[row] = g[row]  (multi-GPU: reduce-scatter first, then tmf_adam_fresh_rows) */

int tmf_version(void);
const char* tmf_last_error(void);

/* Row length (in floats) the kernels use for an n_components-wide factor table: the next
 * size that is 4 floats x a power-of-two number of lanes (<= 64), or a multiple of 256 above that.
 * Returns 0 when n_components is outside [1, 1024]. */
int tmf_padded_ld(int n_components);

/* Same for bf16-stored tables (8 elements per 16-byte lane): the next 8 x power-of-two (<= 512), else 1024. */
int tmf_padded_ld_bf16(int n_components);

/* Scalars of one Keras Adam step at iteration 1 with zero moments, in fp32 - the reference builds
 * a new optimizer every epoch (matrix_factorization.py:176), so this is the whole optimizer state.
 *   alpha = lr*sqrt(1-b2)/(1-b1), one_minus_b1, one_minus_b2, eps = 1e-7 */
typedef struct tmf_adam {
    float alpha, one_minus_b1, one_minus_b2, eps;
} tmf_adam;
tmf_adam tmf_adam_fresh(float lr);

/* A pass over the rows of one side (users or items), cut into segments of at most `chunk`
 * list entries so that heavy rows are shared by several waves:
 *   segment s covers entries [rowptr[seg_row[s]] + seg_chunk[s]*chunk, ... + chunk) of its row;
 *   seg_slab[s] = -1 when the row has a single segment (the epilogue runs in the pass itself),
 *   otherwise the slot of `slab` [n_slab, ld] that receives this segment's partial gradient; rows with
 *   several segments are finished by tmf_combine_rows in slot order (deterministic, atomics-free). */
typedef struct tmf_segments {
    const int64_t* rowptr;    /* [rows + 1] */
    const int32_t* seg_row;   /* [nseg] */
    const int32_t* seg_chunk; /* [nseg] */
    const int32_t* seg_slab;  /* [nseg] */
    int64_t nseg;
    int32_t chunk;
    int32_t row_mod; /* 0, or n_rows when the lists are split by blocks of the OTHER side: list row =
                        block * n_rows + table row (every segment then owns a slab slot) */
} tmf_segments;

/* Index preparation, once per fit() (there is no counterpart in the reference: it gathers from the dense
 * [m, n] score matrix with SparseTensor.indices, loss_graphs.py:47-50; these views are what lets the passes stream).
 *   tmf_csr_build: COO (indices [nnz, 2] int64 pairs in any order, values [nnz]) -> CSR by user, interactions of a user in
 *     ascending item order (the row-major order tf.sparse.SparseTensor is specified in; duplicates keep their input
 *     order): rowptr_u [n_users + 1], col_u / val_u / user_of [nnz].
 *   tmf_csc_perm:  stable order of the CSR entries by item: perm [nnz] (CSR positions), rowptr_i [n_items + 1].
 *   tmf_stable_order_i32: the building block - stable radix sort of int32 keys in [0, n_rows) with their positions,
 *     plus rowptr[r] = first sorted position with key >= r.  sorted_keys may be NULL.
 * workspace: caller-provided device scratch of at least the matching *_workspace_bytes(). */
size_t tmf_csr_build_workspace_bytes(int64_t nnz);
int tmf_csr_build(const int64_t* indices, const float* values, int64_t nnz, int32_t n_users, int32_t n_items,
                  int64_t* rowptr_u, int32_t* col_u, float* val_u, int32_t* user_of, void* workspace,
                  size_t workspace_bytes, void* stream);
size_t tmf_stable_order_workspace_bytes(int64_t n);
int tmf_csc_perm(const int32_t* col_u, int64_t nnz, int32_t n_items, int64_t* rowptr_i, int64_t* perm,
                 void* workspace, size_t workspace_bytes, void* stream);
int tmf_stable_order_i32(const int32_t* keys, int64_t n, int64_t n_rows, int64_t* perm, int32_t* sorted_keys,
                         int64_t* rowptr, void* workspace, size_t workspace_bytes, void* stream);

/* Index structures of the sliced WMRB pass (built once per fit from the static negative table, utils.py:20):
 *   tmf_sort_samples: R_sorted[u, :] = R[u, :] in ascending item order (the order of a user's negatives is immaterial
 *     to the loss, loss_graphs.py:80-86).
 *   tmf_slice_offsets: off[row][b] = first position of the row's ascending ids with id >= b * ceil(n_items / n_slices),
 *     b = 0 .. n_slices (the last one = row length).  Rows have a fixed length `stride` (rowptr NULL: the negatives) or
 *     are CSR rows (the interactions; offsets relative to rowptr[row]).
 *   tmf_wmrb_entry_lists: the item-side lists of the WMRB gradient, split by user block (list row = user block * n_items
 *     + item, blocks of ceil(n_users / user_chunks) users): every list holds the item's positives (ascending CSR
 *     position) followed by the (user, sample) pairs whose negative is the item.  Entry ids: i < nnz = interaction i of
 *     the CSR, nnz + u * S + s = negative s of user u (R_sorted order).  Outputs, E = nnz + n_users * S (< 2^31):
 *       ent_row [E] user of every list entry; ent_id [E] entry id of every list entry (= its index into the weight
 *       buffer [delta | D] of tmf_wsum_pass; stored values <= 0 sit in a dummy list row behind all others);
 *       rowptr_e [user_chunks * n_items + 2]. */
size_t tmf_sort_samples_workspace_bytes(int32_t n_users, int32_t n_samples);
int tmf_sort_samples(const int32_t* R, int32_t n_users, int32_t n_samples, int32_t n_items, int32_t* R_sorted,
                     void* workspace, size_t workspace_bytes, void* stream);
int tmf_slice_offsets(const int32_t* ids, const int64_t* rowptr, int64_t stride, int32_t n_rows, int32_t n_items,
                      int32_t n_slices, int32_t* off, void* stream);
size_t tmf_wmrb_entry_lists_workspace_bytes(int64_t nnz, int32_t n_users, int32_t n_samples);
int tmf_wmrb_entry_lists(const int32_t* user_of, const int32_t* col_u, const float* val_u, int64_t nnz,
                         const int32_t* R_sorted, int32_t n_users, int32_t n_samples, int32_t n_items, int32_t user_chunks,
                         int32_t* ent_row, int32_t* ent_id, int64_t* rowptr_e, void* workspace, size_t workspace_bytes,
                         void* stream);
/* The streams of tmf_wmrb_scores7_f32 / tmf_wmrb_scores7_fill_f32 (below: steps, place, sub_step, sub_place, chunk_sub, sub_fill),
 * built chunk by chunk from the CSR and the item-sorted negative table - no sort, scan or scatter over all entries or all steps.
 * Inputs of all three calls: rowptr_u [n_users + 1], col_u [nnz] ascending inside every user (tmf_csr_build), R_sorted
 * [n_users, n_samples] ascending inside every user (tmf_sort_samples), `width` = items per slice (n_slices = ceil(n_items / width),
 * the n_slices handed to the scores kernel), `slots` = entries per sub-chunk, 1 .. tmf_wmrb_scores7_slots().  n_groups =
 * ceil(n_users / tmf_wmrb_scores7_users_per_group()), n_chunks = n_slices * n_groups, E = nnz + n_users * n_samples.
 * Order rules (an ENTRY: id e < nnz = interaction e, place ~e; e = nnz + u * n_samples + pos = negative pos of user u, place
 * u * n_samples + pos):
 *   chunk = (item / width) * n_groups + u / users_per_group; its entries go by (item, local user, e), so a user's interaction with
 *     an item comes before its negative of that item and repeated ids keep ascending e
 *   sub-chunk j of a chunk = entries [j * slots, (j + 1) * slots) of that order (neighbours may share their border item)
 *   slot = rank inside the sub-chunk by (local user, e); place [E] is written sub-chunk after sub-chunk in slot order
 *   steps: inside a sub-chunk every run of one item, in chunk order, is cut every 4 entries; pads repeat the step's first user and
 *     carry the slot tmf_wmrb_scores7_slots().  fill_order == 0: a sub-chunk's steps in that (item) order; != 0: stably by descending
 *     fill, as tmf_wmrb_scores7_fill_f32 wants them.  steps has n_steps + 1 records: the one behind the last is zero.
 * The calls, in order, each enqueued on `stream`; the host reads two totals in between:
 *   tmf_s7plan_chunks  -> chunk_ent [n_chunks + 1] first entry of every chunk, chunk_sub [n_chunks + 1]; n_sub = chunk_sub[n_chunks]
 *   tmf_s7plan_subs    -> sub_fill [n_sub, 4] steps of fill 4, 3, 2, 1, sub_place, sub_step [n_sub + 1]; n_steps = sub_step[n_sub]
 *   tmf_s7plan_streams -> steps [n_steps + 1] 16-byte records (16-byte aligned), place [E] (NULL: not written, as for a second call
 *                         that only wants the other order of the steps)
 * with chunk_ent, chunk_sub, sub_step handed on unchanged.  The workspace (tmf_s7plan_workspace_bytes(n_chunks) for _chunks,
 * (n_sub) for _subs) is scratch of that call alone.  Limits: n_items < 2^24, nnz < 2^31, n_users * n_samples < 2^31 (int32
 * places), n_chunks < 2^31, n_sub < 2^23 (one launch of 512 threads per sub-chunk; the caller's to check after _chunks).  A null list, a null output, slots outside
 * [1, tmf_wmrb_scores7_slots()], width < 1, n_items outside [1, 2^24), a negative size, a size beyond the limits, a workspace that
 * is null or too small: TMF_E_INVALID and nothing is launched.  n_users == 0 or n_sub == 0 is legal (empty streams). */
size_t tmf_s7plan_workspace_bytes(int64_t n);
int tmf_s7plan_chunks(const int64_t* rowptr_u, const int32_t* col_u, const int32_t* R_sorted, int64_t nnz, int64_t n_users,
                      int32_t n_samples, int32_t n_items, int32_t width, int32_t slots, int64_t* chunk_ent, int32_t* chunk_sub,
                      void* workspace, size_t workspace_bytes, void* stream);
int tmf_s7plan_subs(const int64_t* rowptr_u, const int32_t* col_u, const int32_t* R_sorted, int64_t nnz, int64_t n_users,
                    int32_t n_samples, int32_t n_items, int32_t width, int32_t slots, const int64_t* chunk_ent,
                    const int32_t* chunk_sub, int64_t n_sub, int32_t* sub_fill, int64_t* sub_place, int64_t* sub_step,
                    void* workspace, size_t workspace_bytes, void* stream);
int tmf_s7plan_streams(const int64_t* rowptr_u, const int32_t* col_u, const int32_t* R_sorted, int64_t nnz, int64_t n_users,
                       int32_t n_samples, int32_t n_items, int32_t width, int32_t slots, const int64_t* chunk_ent,
                       const int32_t* chunk_sub, int64_t n_sub, const int64_t* sub_step, int64_t n_steps, int32_t fill_order,
                       void* steps, int32_t* place, void* stream);

/* K1+K2 / K3: one side of an MSE epoch (loss_graphs.py:47-52 forward; tape.gradient
 * matrix_factorization.py:170-171; Adam :176) evaluated sparsely:
 *   for every entry k of row i:  p = <X_old[i], Y_old[other[k]]>, e = val[k] - p,
 *   loss += e*e, g[i] += (-2e) * Y_old[other[k]]; then the epilogue `epi` writes X_out[i].
 * Call once with (X=U, Y=V, CSR by user) and once with (X=V, Y=U, CSC by item); both read the
 * PRE-update tables.  loss_part (optional, [nseg]) receives the per-segment sum of e*e. */
int tmf_mse_pass_f32(const tmf_segments* seg, const int32_t* other, const float* val,
                     const float* X_old, const float* Y_old, float* X_out, float* slab,
                     float* loss_part, int n_components, int epi, tmf_adam adam, void* stream);

/* One epoch of KLDivergenceLoss (loss_graphs.py:91-122 forward - two masks, tf.nn.moments of the stored scores of either class,
 * 1 - Normal(mu- - mu+, sqrt(v+ + v-)).cdf(0); matrix_factorization.py:158-176 - the serial scores, tape.gradient, Adam)
 * evaluated sparsely.  Class "+" = entries with val > 0, class "-" = entries with val <= 0 (stored zeros included); a NaN value is
 * in neither and gets weight 0.  With N_c, mu_c, v_c the count, mean and population variance of p_k = <U[u_k], V[i_k]> over
 * class c, sigma = sqrt(v+ + v-), z = (mu+ - mu-) / sigma and phi = exp(-z^2 / 2) / sqrt(2 pi):
 *   loss = erfc(z / sqrt 2) / 2 (one scalar),   d loss / d p_k = a_c + b_c (p_k - mu_c),
 *   a+ = -phi / (sigma N+),  a- = +phi / (sigma N-),  b_c = phi (mu+ - mu-) / (sigma^3 N_c).
 * tmf_kl_moments_*: walks the user-side segments (X = U, Y = V, CSR by user) and writes, per segment, part[s][0..5] = N+, N-,
 *   sum p+, sum p-, sum p^2+, sum p^2- - fp64 sums in a fixed order, no atomics; no table is written.  part: [nseg, 6] fp64,
 *   16-byte aligned.
 * tmf_kl_coeffs: one workgroup adds the nseg partials in a fixed order in fp64 and writes the loss into loss_out[0] and
 *   coef[0..5] = a+, b+, mu+, a-, b-, mu- (fp64, device memory; nothing comes back to the host).  An empty class or sigma = 0
 *   gives NaN / inf, as the reference's arithmetic does.
 * tmf_kl_pass_*: the contract of tmf_mse_pass_* with `coef` in place of loss_part and the weight a_c + b_c (p_k - mu_c), p_k
 *   recomputed from the gathered row, in place of -2 (val - p); padded slots and NaN values weigh 0.  Call once with (X = U,
 *   Y = V, CSR by user) and once with (X = V, Y = U, CSC by item); both read the PRE-update tables; rows of several segments
 *   are finished by tmf_combine_rows_*.
 * Null tables or a bad `epi`: TMF_E_INVALID; nseg == 0: TMF_OK; nothing is launched in either case. */
int tmf_kl_moments_f32(const tmf_segments* seg, const int32_t* other, const float* val, const float* X_old,
                       const float* Y_old, double* part, int n_components, void* stream);
int tmf_kl_coeffs(const double* part, int64_t nseg, double* loss_out, double* coef, void* stream);
int tmf_kl_pass_f32(const tmf_segments* seg, const int32_t* other, const float* val, const float* X_old,
                    const float* Y_old, float* X_out, float* slab, const double* coef, int n_components, int epi,
                    tmf_adam adam, void* stream);

/* One side of a LogisticLoss epoch (mf/loss_graphs.py LogisticLoss: the pointwise logistic loss over signed feedback - an
 * extension, the reference has no such loss) evaluated sparsely: the contract of tmf_mse_pass_* with another coefficient.
 *   for every entry k of row i:  p = <X_old[i], Y_old[other[k]]>,  y = val[k] > 0 ? +1 : -1 (a stored 0 is a negative: the
 *   class split of tmf_kl_*; a NaN value is a negative too),  w = weighted ? |val[k]| : 1,
 *   loss += w log(1 + exp(-y p)),  g[i] += c Y_old[other[k]] with c = -y w sigma(-y p);  then the epilogue `epi` writes X_out[i].
 * fp32 arithmetic, stable for every finite p: with x = -y p and t = exp(-|x|), sigma(x) = (x >= 0 ? 1 : t) / (1 + t) and
 * softplus(x) = max(x, 0) + log1p(t) - no overflow and no NaN beyond |p| = 88.7, and c = -+w / 2 exactly at p = 0.
 * Call once with (X = U, Y = V, CSR by user) and once with (X = V, Y = U, CSC by item); both read the PRE-update tables.
 * loss_part (optional, [nseg]) receives the per-segment sum of w softplus(-y p); with loss_part == NULL no logarithm is
 * computed.  Rows of several segments go to `slab` and are finished by tmf_combine_rows_* with the same epi.  `weighted`
 * (0 | non-zero) stands before the stream; the other arguments are tmf_mse_pass_*'s.
 * No atomics and a fixed order of additions: results are bit-identical from call to call.
 * Null tables or lists, a bad `epi`, n_components outside [1, 1024]: TMF_E_INVALID; nseg == 0: TMF_OK; nothing is launched in
 * either case. */
int tmf_logistic_pass_f32(const tmf_segments* seg, const int32_t* other, const float* val, const float* X_old,
                          const float* Y_old, float* X_out, float* slab, float* loss_part, int n_components, int epi,
                          tmf_adam adam, int weighted, void* stream);

/* Weighted row-gather-sum pass (item side of WMRB, matrix_factorization.py:170-171 through
 * loss_graphs.py:80-88):  g[i] = sum over entries e of row i of  wbuf[ent_w[e]] * T[ent_row[e]]
 * (entries with weight exactly 0 are skipped), then the epilogue writes X_out[i]. */
int tmf_wsum_pass_f32(const tmf_segments* seg, const int32_t* ent_row, const int32_t* ent_w,
                      const float* wbuf, const float* T, const float* X_old, float* X_out,
                      float* slab, int n_components, int epi, tmf_adam adam, void* stream);

/* Row-stationary form of tmf_wsum_pass + tmf_combine_rows over user-blocked lists (speed only): the lists are those of
 * tmf_wmrb_entry_lists with `n_blocks` user blocks - list row = block * n_rows + i, rowptr [n_blocks * n_rows + 1] - but a
 * lane group owns a few consecutive output rows i, keeps their sums in registers and walks the blocks itself: no slab, no
 * combine.  g[i] = sum over blocks (ascending) and list entries e of wbuf[ent_w[e]] * T[ent_row[e]], then the epilogue.
 * The rows are launched `rows_per_launch` at a time (a multiple of tmf_wsum_rows4_rows_per_group(); all workgroups of a
 * launch resident together); workspace (optional): tmf_wsum_rows4_workspace_bytes() of device memory for the per-block
 * rendezvous counters, zeroed by the call.  Rows of at least 16 lanes. */
int tmf_wsum_rows4_rows_per_group(int n_components, int bf16);
size_t tmf_wsum_rows4_workspace_bytes(int32_t n_rows, int32_t n_blocks, int32_t rows_per_launch);
int tmf_wsum_rows4_f32(const int64_t* rowptr, int32_t n_rows, int32_t n_blocks, const int32_t* ent_row, const int32_t* ent_w,
                       const float* wbuf, const float* T, const float* X_old, float* X_out, int n_components, int epi,
                       tmf_adam adam, int32_t rows_per_launch, void* workspace, size_t workspace_bytes, void* stream);

/* BALANCED row-stationary form (round 5; speed only): what the lane groups own are VIRTUAL rows - (output row, part p of P), listed
 * in (row, part) order - so that a row with far more list entries than the average (a popular item: one entry per user against
 * 1,400 on average at config 5) is cut into P parts of about the average size and every lane group walks about the same number of
 * entries.  In block t part p of row i takes the entries [b + p L / P, b + (p + 1) L / P) of that block's list [b, b + L).
 *   vr_item / vr_part / vr_nparts [n_vrows + 1]: output row, part and number of parts of every virtual row; the last element is
 *   the sentinel (n_rows, 0, 1);  vr_slot [n_vrows]: -1 = the row is whole (P = 1) and finished by the epilogue, else the slab slot
 *   its partial sum goes to - the caller then finishes the cut rows with tmf_combine_rows: slots of a row consecutive, in part
 *   order.  A fixed order of additions: results are bit-reproducible; against tmf_wsum_rows4 / tmf_wsum_pass equal to rounding.
 * rows_per_launch counts virtual rows (a multiple of tmf_wsum_rows4_rows_per_group()). */
size_t tmf_wsum_rows5_workspace_bytes(int32_t n_vrows, int32_t n_blocks, int32_t rows_per_launch);
int tmf_wsum_rows5_f32(const int64_t* rowptr, int32_t n_rows, int32_t n_blocks, const int32_t* ent_row, const int32_t* ent_w,
                       const float* wbuf, const float* T, const float* X_old, float* X_out, float* slab, const int32_t* vr_item,
                       const int32_t* vr_part, const int32_t* vr_nparts, const int32_t* vr_slot, int32_t n_vrows, int n_components,
                       int epi, tmf_adam adam, int32_t rows_per_launch, void* workspace, size_t workspace_bytes, void* stream);

/* Finishes the rows that tmf_*_pass cut into several segments: g[row] = sum of its slab slots
 * [slab_beg[i], slab_beg[i+1]) in order, then the epilogue. */
int tmf_combine_rows_f32(const int32_t* long_rows, const int64_t* slab_beg, int64_t n_long,
                         const float* slab, const float* X_old, float* X_out, int n_components,
                         int epi, tmf_adam adam, void* stream);

/* K4+K5: user side of a WMRB epoch for users [0, n_users) in ONE kernel (matrix_factorization.py:153-154 sampled
 * and serial scores, loss_graphs.py:74-88, gradient w.r.t. U, Adam :176) - the form for catalogs whose V table the L2s
 * hold and sample counts whose scores fit LDS (tmf_wmrb_user_pass_fits); everything else takes the sliced pass below.
 *   R [n_users, S] int32 static negative table (utils.py:20), c = n_items / n_samples (ctor ints);
 *   writes delta [nnz] (d loss / d p_k, 0 for non-positive entries), D [n_users, S],
 *   loss_part [n_users] (sum of log(1+M_k) over the user's positives), pos_part [n_users] (#positives),
 *   and U_out via the epilogue. */
int tmf_wmrb_user_pass_f32(const int64_t* rowptr, const int32_t* col, const float* val,
                           const int32_t* R, int32_t n_users, int32_t S, float c,
                           const float* U_old, const float* V_old, float* U_out, float* delta,
                           float* D, float* loss_part, float* pos_part,
                           int n_components, int epi, tmf_adam adam, void* stream);
/* 1 when the scores and D of one user (n_samples of them) fit the 160 KB of LDS next to the kernel's other buffers. */
int tmf_wmrb_user_pass_fits(int32_t n_samples, int n_components);

/* Sliced form of the same user pass (speed only - same contract): the catalog is walked in n_slices slices of
 * ~4 MB of V rows with a slice-major grid, so the row gathers of the resident workgroups hit the XCD L2s; it also has
 * no limit on n_samples, and its hinge step costs O((S + P_u) log P_u) per user instead of O(P_u S).  The lists: */
typedef struct tmf_slice_lists {
    const int32_t* R_sorted;  /* [n_users, n_samples] negatives, ascending item id per user (tmf_sort_samples) */
    const int32_t* slice_off; /* [n_users, n_slices + 1] (tmf_slice_offsets on R_sorted) */
    const int64_t* rowptr;    /* [n_users + 1] CSR of the interactions, ascending item id inside a user (tmf_csr_build) */
    const int32_t* col;       /* [nnz] */
    const int32_t* pos_off;   /* [n_users, n_slices + 1] (tmf_slice_offsets on col with rowptr) */
    int32_t n_users, n_samples, n_slices;
    /* Window of the catalog a launch covers (item-row-sharded V, one window of rows resident at a time): slices
     * [slice_begin, slice_begin + slice_count) and the V pointer of the call addresses item row `item_base` (the first row
     * of the window).  All three 0 = the whole catalog. */
    int32_t slice_begin, slice_count, item_base;
    /* Bit set (this field was `xcd_major` = 0 | 1 up to version 202, so older callers keep their meaning):
     *   TMF_SLICE_XCD_MAJOR (1)      block order of the slice kernels (speed only): clear = slice-major (every resident workgroup
     *                                walks the same slice, each XCD L2 holds a copy of it), set = XCD-major (the XCD of block b - b mod 8
     *                                under the observed round-robin placement - walks the slices slice_begin + 8 i + (b mod 8): eight
     *                                different slices resident, one per L2);
     *   TMF_SLICE_N_ITEMS_STATED (2) `n_items` below is meaningful.  The struct is 72 bytes: 5 pointers + 8 int32.  Up to version 201
     *                                it ended after this field (68 bytes + 4 of tail padding), so a caller built against that
     *                                header passes indeterminate bytes where n_items now sits: they are ignored unless this bit says
     *                                the caller filled them in. */
    int32_t flags;
    /* Items in the catalog the ids of R_sorted / col index (the rows of V); counts only with TMF_SLICE_N_ITEMS_STATED.  Speed
     * only: when stated and n_items * row bytes < 2^32, tmf_wmrb_scores3 addresses V with 32-bit offsets (one instruction per row
     * address).  TMF_CHECK_IDS=1 in the environment makes the call verify (synchronously) that every id is below it. */
    int32_t n_items;
} tmf_slice_lists;
#define TMF_SLICE_XCD_MAJOR 1
#define TMF_SLICE_N_ITEMS_STATED 2
/* Kernels, called in this order on one stream (tables float (_f32) or bf16 (_bf16) rows as void*; sp / p / D / delta /
 * part / w_ent are fp32):
 *   tmf_wmrb_scores3_*  sp[u, s] = <U[u], V[R_sorted[u, s]]>, p[k] = <U[u_k], V[col[k]]>         (slice-major grid)
 *   tmf_wmrb_hinge2     delta [nnz], D [n_users, n_samples] (R_sorted order), loss_part [n_users]; reads no table
 *   tmf_wmrb_gradu3_*   part[slice][u] = sum_{s in slice} D[u, s] V[R_sorted[u, s]] + sum_{k in slice} delta_k V[col[k]]
 *                       per_slice_launches = 0: one launch, part is [n_slices * n_users, ld], finish gets n_slices;
 *                       per_slice_launches = 1: one launch per slice adding into ONE [n_users, ld] layer (memory-light;
 *                       finish is then called with n_slices = 1); the first slice launched overwrites the layer;
 *                       per_slice_launches = 3: one launch per ROUND of eight slices into EIGHT layers (part is
 *                       [8 * n_users, ld]; the slice slice_begin + 8 i + x goes to layer x; finish gets min(8, slices));
 *                       per_slice_launches = 2: the same as 1, but the first slice launched adds to the layer as well (the
 *                       later windows of a windowed pass)
 *   tmf_wmrb_finish_*   U_out[u] = epilogue(sum_slice part[slice][u]); with TMF_EPI_GRAD, U_out == part is allowed (the
 *                       layers are summed in place into layer 0) */
int tmf_wmrb_scores3_f32(const tmf_slice_lists* lists, const void* U, const void* V, float* sp, float* p,
                         int n_components, void* stream);
int tmf_wmrb_scores3_bf16(const tmf_slice_lists* lists, const void* U, const void* V, float* sp, float* p,
                          int n_components, void* stream);
/* Row-stationary form of scores3 (speed only - the same sp / p up to the order of the fp32 sum inside a dot product; exact on
 * dyadic data): for catalogs far beyond the L2s, where a (user, slice) visit holds a handful of rows and scores3 is bound by what
 * every visit reads besides them (matrix_factorization.py:153-154 and utils.py:94-105 are what both compute).  A workgroup owns
 * tmf_wmrb_scores5_users_per_workgroup() consecutive users, keeps their rows in LDS and walks ONE flat stream of its (user, item)
 * pairs - negatives and interactions alike, ordered by item (slice) so that all workgroups of a launch gather from the same
 * cache-sized window of V at any time:
 *   ids [E8]     (local user << 24) | item            (E8 = every workgroup's entries padded to a multiple of 8)
 *   outs [E8]    >= 0: index into sp ([n_users, n_samples] flat); < 0: ~index into p ([nnz]); INT32_MIN: padding entry
 *   wg_ptr [n_wg + 1]  first entry of every workgroup's stream (multiples of 8), n_wg = ceil(n_users / users_per_workgroup)
 * wgs_per_launch <= 0: one workgroup per CU (all workgroups of a launch resident, walking the catalog at the same pace).
 * Pacing (optional, speed only): wstart [n_wg, n_windows + 1] = the first step (8 entries) of every catalog window in every
 * workgroup's stream (wstart[., n_windows] = its steps) and a workspace of tmf_wmrb_scores5_workspace_bytes() (zeroed by the
 * call): a workgroup then starts window w only when the workgroups sharing its XCD have completed window w - lag - 1 (bounded
 * waits), so that the rows being gathered span lag + 1 windows.  NULL = every workgroup runs freely.
 * Needs rows of 32 lanes (fp32 65..128, bf16 129..256 components), n_items < 2^24 and a V table below 4 GB:
 * tmf_wmrb_scores5_supported(). */
int tmf_wmrb_scores5_users_per_workgroup(void);
int tmf_wmrb_scores5_supported(int n_components, int bf16, int64_t n_items);
size_t tmf_wmrb_scores5_workspace_bytes(int64_t n_wg, int32_t n_windows, int wgs_per_launch);
int tmf_wmrb_scores5_f32(const int32_t* ids, const int32_t* outs, const int64_t* wg_ptr, int64_t n_wg, int64_t n_users,
                         int64_t n_items, const void* U, const void* V, float* sp, float* p, int n_components,
                         int wgs_per_launch, const int32_t* wstart, int32_t n_windows, int lag, void* workspace,
                         size_t workspace_bytes, void* stream);
int tmf_wmrb_scores5_bf16(const int32_t* ids, const int32_t* outs, const int64_t* wg_ptr, int64_t n_wg, int64_t n_users,
                          int64_t n_items, const void* U, const void* V, float* sp, float* p, int n_components,
                          int wgs_per_launch, const int32_t* wstart, int32_t n_windows, int lag, void* workspace,
                          size_t workspace_bytes, void* stream);
/* Flat streams on the slice-major grid (round 5; speed only - the same sp / p as tmf_wmrb_scores3 up to the order of the fp32 sum
 * inside a dot product, exact on dyadic data): one workgroup per CHUNK = (item slice, group of tmf_wmrb_scores6_users_per_group()
 * consecutive users); the group's rows are held in LDS and the chunk's entries are one contiguous piece of
 *   ids [E8]   (user - first user of the group) << 24 | item      outs [E8]   as for tmf_wmrb_scores5
 *   chunk_ptr [n_slices * n_groups + 1]   first entry of chunk slice * n_groups + group (every chunk padded to a multiple of 8)
 * - interactions first, then negatives, each by user and item - so a (user, slice) visit costs no offsets, no row of U and no
 * dependent round trip of its own.  The slices only order the stream and the grid (the kernel never sees their bounds): any
 * partition of the item ids into n_slices ascending ranges will do; ~4 MB of V rows each keeps a slice in the XCD L2s.
 * Same limits as tmf_wmrb_scores5: rows of 32 lanes, n_items < 2^24, V below 4 GB (tmf_wmrb_scores6_supported). */
int tmf_wmrb_scores6_users_per_group(void);
int tmf_wmrb_scores6_supported(int n_components, int bf16, int64_t n_items);
int tmf_wmrb_scores6_f32(const int32_t* ids, const int32_t* outs, const int64_t* chunk_ptr, int64_t n_groups, int32_t n_slices,
                         int64_t n_users, int64_t n_items, const void* U, const void* V, float* sp, float* p, int n_components,
                         void* stream);
int tmf_wmrb_scores6_bf16(const int32_t* ids, const int32_t* outs, const int64_t* chunk_ptr, int64_t n_groups, int32_t n_slices,
                          int64_t n_users, int64_t n_items, const void* U, const void* V, float* sp, float* p, int n_components,
                          void* stream);
/* Item runs (speed only - the same sp / p as tmf_wmrb_scores3 up to the order of the fp32 sum inside a dot product, exact on dyadic
 * data): one workgroup per chunk = (item slice, group of tmf_wmrb_scores7_users_per_group() consecutive users) as for
 * tmf_wmrb_scores6, the group's rows in LDS - but the chunk's entries come by ITEM, so the users of a group that need a row of V
 * share one load of it.
 *   steps [n_steps] 16-byte records {int32 item; uint8 local_user[4]; uint16 slot[4]}: one item and up to 4 users of the group
 *                   that need it; a short step is padded with a valid local user and the slot tmf_wmrb_scores7_slots()
 *   place [n_entries]      where the score of a slot goes: >= 0 -> sp[place], < 0 -> p[~place]
 *   sub_step / sub_place [n_sub + 1]   first step / first place of every SUB-CHUNK: the steps whose scores fill one LDS buffer of
 *                   at most tmf_wmrb_scores7_slots() slots; the buffer is then stored slot i -> place[sub_place[sub] + i]
 *   chunk_sub [n_slices * n_groups + 1]   first sub-chunk of chunk slice * n_groups + group
 * Every (user, item) pair of the epoch is in exactly one non-pad slot.  fp32 rows of 65..128 components, n_items < 2^24, V below
 * 4 GB (tmf_wmrb_scores7_supported; 0 for everything else, bf16 included).
 * tmf_wmrb_scores7_f32 deals the steps of a sub-chunk round-robin to its lane groups and computes all 4 slots of every step, pads
 * included (their scores land behind the buffer); it is correct for the steps of a sub-chunk in ANY order.
 * tmf_wmrb_scores7_fill_f32 wants the steps of every sub-chunk by descending FILL (= slots that are no pads; a step's entries come
 * first, its pads behind them) and two tables that say so:
 *   sub_fill [n_sub, 4]    the sub-chunk's steps of fill 4, 3, 2, 1 (they sum to its steps)
 *   sub_wave [n_sub, tmf_wmrb_scores7_waves() + 1]   first step, counted from the sub-chunk's first, of every wave's contiguous range:
 *                   starts at 0, ends at the sub-chunk's steps, never descends; an empty range leaves the wave idle
 * A wave cuts its range at the class borders and runs each part with a loop that computes slots k < fill only: a pad slot costs
 * nothing.  The same scores, bit for bit: a score does not depend on the step, lane group or loop it is computed in. */
int tmf_wmrb_scores7_users_per_group(void);
int tmf_wmrb_scores7_waves(void);
int tmf_wmrb_scores7_fill_f32(const void* steps, const int32_t* place, const int64_t* sub_step, const int64_t* sub_place,
                              const int32_t* chunk_sub, const int32_t* sub_wave, const int32_t* sub_fill, int64_t n_groups,
                              int32_t n_slices, int64_t n_users, int64_t n_items, const void* U, const void* V, float* sp, float* p,
                              int n_components, void* stream);
int tmf_wmrb_scores7_slots(void);
int tmf_wmrb_scores7_supported(int n_components, int bf16, int64_t n_items);
int tmf_wmrb_scores7_f32(const void* steps, const int32_t* place, const int64_t* sub_step, const int64_t* sub_place,
                         const int32_t* chunk_sub, int64_t n_groups, int32_t n_slices, int64_t n_users, int64_t n_items,
                         const void* U, const void* V, float* sp, float* p, int n_components, void* stream);
int tmf_wmrb_hinge2(const int64_t* rowptr, const float* val, const float* p, const float* sp, int32_t n_users,
                    int32_t n_samples, float c, float* delta, float* D, float* loss_part, void* stream);
/* The same with the order in which the waves take the users (a permutation of 0 .. n_users - 1, or NULL = 0, 1, 2 ...): a user
 * costs one pass per 255 interactions, so the few with thousands should start first, not last.  Speed only - every user is
 * computed by itself and the outputs do not depend on the order. */
int tmf_wmrb_hinge2_ordered(const int64_t* rowptr, const float* val, const float* p, const float* sp, int32_t n_users,
                            int32_t n_samples, float c, float* delta, float* D, float* loss_part, const int32_t* user_order,
                            void* stream);
/* BPRLoss (an extension) in the place of tmf_wmrb_hinge2_ordered, same layout of every argument: for the stored values > 0 of user u,
 * x_ks = sp[u, s] - p[k]:  delta[k] = -(1 / S) sum_s sigmoid(x_ks) (0 for a stored value <= 0),  D[u, s] = (1 / S) sum_k
 * sigmoid(x_ks),  loss_part[u] = (1 / S) sum_k sum_s softplus(x_ks) - the pairwise logistic loss -log sigmoid(p[k] - sp[u, s]),
 * averaged over the user's row of the negative table; the epoch's loss is the sum of loss_part over the number of positives.
 * Every element of delta [nnz], D [n_users, n_samples] and loss_part [n_users] is overwritten, whatever the buffers held.  Reads no
 * table; O(P_u S) exponentials per user.  n_users = 0 is legal, and so are NULL val / p / delta for a table without interactions.
 * No atomics; the outputs are bit-identical from run to run and do not depend on user_order (speed only: heavy users first).
 * Finite for every finite score; +inf in sp gives loss inf and sigmoid 1; a NaN stays inside its user. */
int tmf_bpr_pairs(const int64_t* rowptr, const float* val, const float* p, const float* sp, int32_t n_users, int32_t n_samples,
                  float* delta, float* D, float* loss_part, const int32_t* user_order, void* stream);
/* WARPLoss (an extension) in the same place, same layout of every argument, + the catalog size: for the stored values > 0 of user u,
 * t_k = fl(p[k] - 1):  s* = the first s with sp[u, s] > t_k (strict, in table order; a NaN never violates),  N = s* + 1,
 * w = log(max(1, floor((n_items - 1) / N))) - 0 without a violator or with N > n_items - 1;  delta[k] = -w (0 for a stored value
 * <= 0),  D[u, s*] += w,  loss_part[u] = sum_k w (1 - p[k] + sp[u, s*]); the epoch's loss is the sum of loss_part over the number
 * of positives.  Every element of delta [nnz], D [n_users, n_samples] and loss_part [n_users] is overwritten, whatever the
 * buffers held.  Reads no table; O(S + P log S) per user (a prefix maximum of the row and a binary search per positive), rows of
 * any length >= 1.  n_users = 0 is legal, and so are NULL val / p / delta for a table without interactions.  No atomics; the
 * outputs are bit-identical from run to run and do not depend on user_order (speed only: heavy users first). */
int tmf_warp_pairs(const int64_t* rowptr, const float* val, const float* p, const float* sp, int32_t n_users, int32_t n_samples,
                   int32_t n_items, float* delta, float* D, float* loss_part, const int32_t* user_order, void* stream);
/* The same with sp and D in another order than the table's (the sliced pass keeps every user's samples sorted by item, and this
 * loss depends on their order): rank[u, pos] in [0, n_samples) is the table index of the sample at place pos of user u's row - a
 * permutation of every row, 16 bits each (n_samples <= 65536).  Trials run in table order; D[u, pos] is the weight of the sample
 * at place pos.  The bits of tmf_warp_pairs on the rows in table order, moved to their places. */
int tmf_warp_pairs_ranked(const int64_t* rowptr, const float* val, const float* p, const float* sp, const uint16_t* rank,
                          int32_t n_users, int32_t n_samples, int32_t n_items, float* delta, float* D, float* loss_part,
                          const int32_t* user_order, void* stream);
/* KOSWARPLoss (an extension), the weights: omega[j] = the probability that the k'-th best of n' uniform draws with replacement from
 * the P stored values > 0 of the entry's user is entry j - n' = min(n, P), k' = min(k, n'), 1 <= k <= n <= 64.  With a_j / b_j the
 * number of the user's positives whose score p is above / not below p[j] (compared in fp32; a NaN orders below -inf and ties with
 * the other NaNs) and B(q) = sum_{i < k'} C(n', i) q^i (1 - q)^(n' - i), B(0) = 1, B(1) = 0:
 * omega[j] = (B(a_j / P) - B(b_j / P)) / (b_j - a_j), B in fp64, rounded to fp32 once; 0 for a stored value <= 0.  A tie block shares
 * its probability equally, the weights of a user with P >= 1 sum to 1.  Every element of omega [nnz] is overwritten, whatever the
 * buffer held.  Reads no table; one LDS sort of the user's scores and two bisections per entry, rows of any length (a row of more
 * than 2048 positives is taken in segments).  n_users = 0 is legal, and so are NULL val / p / omega for a table without
 * interactions.  No atomics; the outputs are bit-identical from run to run and do not depend on user_order (speed only). */
int tmf_kos_weights(const int64_t* rowptr, const float* val, const float* p, int32_t n_users, int32_t k, int32_t n, float* omega,
                    const int32_t* user_order, void* stream);
/* tmf_warp_pairs (rank = NULL) or tmf_warp_pairs_ranked (with rank) with a weight per stored entry: w' = fl(omega[k] w), one fp32
 * rounding, stands in w's place everywhere - delta[k] = -w', D[u, s*] += w', loss_part[u] = sum_k w' (1 - p[k] + sp[u, s*]), and an
 * entry with w' = 0 (or not > 0) takes no part.  omega [nnz] is required.  omega = 1 everywhere gives the bits of the two above. */
int tmf_warp_pairs_kos(const int64_t* rowptr, const float* val, const float* p, const float* sp, const uint16_t* rank,
                       const float* omega, int32_t n_users, int32_t n_samples, int32_t n_items, float* delta, float* D,
                       float* loss_part, const int32_t* user_order, void* stream);
/* SampledSoftmaxLoss (an extension) in the same place, the arguments of tmf_wmrb_hinge2_ordered in their layout: for the stored
 * values > 0 of user u, with M = max_s sp[u, s], e_s = exp(sp[u, s] - M), Z = sum_s e_s, m = max(p[k], M), t = exp(M - m),
 * b = c Z t and den = exp(p[k] - m) + b:  loss_k = log(den) + (m - p[k]) = -log(exp(p[k]) / (exp(p[k]) + c sum_s exp(sp[u, s]))),
 * delta[k] = -b / den (0 for a stored value <= 0),  D[u, s] = e_s sum_k c t / den,  loss_part[u] = sum_k loss_k; the epoch's loss
 * is the sum of loss_part over the number of positives.  c = 1, or n_items / n_samples for the uniform-sampling estimate of the
 * full-catalog partition.  sp and D may keep a user's samples in any order: the loss does not depend on it.  Every element of
 * delta [nnz], D [n_users, n_samples] and loss_part [n_users] is overwritten, whatever the buffers held; a user without a value
 * > 0 gets zeros.  Reads no table; one exponential per (user, sample) and two per positive, rows of any length >= 1 (the first 1024
 * samples of a row stay in registers between the read and the write).  n_users = 0 is legal, and so are NULL val / p / delta for a
 * table without interactions.  No atomics; the outputs are bit-identical from run to run and do not depend on user_order (speed
 * only: heavy users first).  Finite for every finite score; a NaN or an infinity stays inside its user. */
int tmf_softmax_pairs(const int64_t* rowptr, const float* val, const float* p, const float* sp, int32_t n_users, int32_t n_samples,
                      float c, float* delta, float* D, float* loss_part, const int32_t* user_order, void* stream);
/* The logQ correction of SampledSoftmaxLoss (an extension; TMF_VERSION stays 203: nothing that existed changes).
 * tmf_softmax_pairs_offset is tmf_softmax_pairs - the same kernel body, a template parameter apart - on the corrected scores
 * x[u, s] = fl(sp[u, s] - off[u, s]), one fp32 subtraction each: M, e_s, Z and D are those of x, p[k] stays raw, and D is the
 * derivative with respect to sp as well.  off: fp32 [n_users, n_samples] in the slot order of sp, read once where sp is read once
 * (tile 0 of the corrected scores stays in registers from that read to the D write; a longer row reads both streams again), both
 * streams' loads of a tile in flight together.  Everything else as above: every output element overwritten, zeros for a user
 * without a value > 0 (neither sp nor off of a user without entries is read), no atomics, every sum in one fixed order, bits
 * independent of user_order; off = 0 gives the bits of tmf_softmax_pairs.  A NaN or an infinity among a user's offsets stays
 * inside that user.  n_users = 0 is TMF_OK; a negative count, n_samples = 0 with users, or a null rowptr / sp / off / D:
 * TMF_E_INVALID before any launch.
 * tmf_slot_offsets builds that table: off[j] = ell[R[j]] over the flat [n_users * n_samples] table R of item ids, which the caller
 * has checked to lie in [0, n_items) - ell: fp32 [n_items].  16-byte pieces where R and off are both 16-byte aligned, element by
 * element otherwise and behind the last whole piece.  Once per table, not per epoch.  n_users = 0 or n_samples = 0: TMF_OK, no
 * launch; a negative count or a null ell / R / off with samples: TMF_E_INVALID before any launch.  Plain vector loads and stores. */
int tmf_softmax_pairs_offset(const int64_t* rowptr, const float* val, const float* p, const float* sp, const float* off,
                             int32_t n_users, int32_t n_samples, float c, float* delta, float* D, float* loss_part,
                             const int32_t* user_order, void* stream);
int tmf_slot_offsets(const float* ell, int32_t n_items, const int32_t* R, int64_t n_users, int32_t n_samples, float* off,
                     void* stream);
int tmf_wmrb_gradu3_f32(const tmf_slice_lists* lists, const float* D, const float* delta, const void* V, float* part,
                        int per_slice_launches, int n_components, void* stream);
int tmf_wmrb_gradu3_bf16(const tmf_slice_lists* lists, const float* D, const float* delta, const void* V, float* part,
                         int per_slice_launches, int n_components, void* stream);
/* Row-stationary form of gradu3 + finish in one kernel (speed only - same result up to the order of the fp32 sum over a
 * user's slices, which is ascending here too): every lane group owns a few users, keeps their gradient rows in registers
 * and walks all slices itself; U_out[u] = epilogue(sum_slice ...).  The users are launched in blocks of `users_per_launch`
 * (all workgroups of a block resident together, so they walk the slices in loose lockstep and the slice stays in the L2s).
 * For catalogs far beyond the L2s, where a (user, slice) range holds a handful of rows. */
int tmf_wmrb_gradu4_supported(int n_components, int bf16);   /* rows of at least 8 lanes (r > 28 fp32, r > 56 bf16) */
size_t tmf_wmrb_gradu4_workspace_bytes(int32_t n_users, int32_t n_slices, int32_t users_per_launch);
/* workspace (optional, device memory): one int per (launch, slice), zeroed by the call; with it the workgroups of a launch
 * rendezvous once per slice (bounded wait, speed only) so that they stay within two slices of each other. */
int tmf_wmrb_gradu4_f32(const tmf_slice_lists* lists, const float* D, const float* delta, const void* V, const void* U_old,
                        void* U_out, int n_components, int epi, tmf_adam adam, int32_t users_per_launch, void* workspace,
                        size_t workspace_bytes, void* stream);
int tmf_wmrb_gradu4_bf16(const tmf_slice_lists* lists, const float* D, const float* delta, const void* V, const void* U_old,
                         void* U_out, int n_components, int epi, tmf_adam adam, int32_t users_per_launch, void* workspace,
                         size_t workspace_bytes, void* stream);
int tmf_wmrb_finish_f32(const float* part, int32_t n_slices, int32_t n_users, const void* U_old, void* U_out,
                        int n_components, int epi, tmf_adam adam, void* stream);
int tmf_wmrb_finish_bf16(const float* part, int32_t n_slices, int32_t n_users, const void* U_old, void* U_out,
                         int n_components, int epi, tmf_adam adam, void* stream);

/* K6 standalone: W[rows] = fresh-Adam(W[rows], G[rows]) in place over n_rows x ld floats. */
int tmf_adam_fresh_rows_f32(float* W, const float* G, int64_t n_rows, int n_components,
                            tmf_adam adam, void* stream);

/* BiasedLinearEmbedding over indicator features (embedding_graphs.py:41-58): the effective table is E = W + 1 b^T with a
 * trainable [1, r] bias b.  The passes read E and, under TMF_EPI_GRAD, write G = dL/dE = dL/dW [n_rows, ld]; dL/db is the column
 * sum of G, and W, b take the same fresh-Adam step (matrix_factorization.py:173-176).  fp32 tables only.  Per epoch and side:
 * the pass with TMF_EPI_GRAD, tmf_bias_colsum_f32 (colsum = NULL), tmf_bias_adam_f32, tmf_adam_bias_rows_f32.
 *
 *   tmf_bias_colsum_part_rows  rows P of the workspace `part` [P, ld] fp64 for a table of n_rows rows (>= 1; 0 for n_rows < 0).
 *   tmf_bias_colsum_f32        part[p][c] = sum of G[i][c] over the p-th block of rows (a fixed partition, fp64 accumulators, no
 *                              atomics).  With colsum != NULL also colsum[c] = sum_p part[p][c] for c < n_components and 0 for the
 *                              padding columns, [ld] fp64, summed in a fixed order: bit-identical from run to run.  The padding
 *                              columns of G may hold anything.  n_rows = 0 gives zeros.  part_rows must be what
 *                              tmf_bias_colsum_part_rows returns for n_rows.
 *   tmf_bias_adam_f32          g_b[c] = fp32(sum_p part[p][c]) (the same fixed order, rounded once), stored in g_out [ld] when it is
 *                              not NULL, and b[c] = fresh-Adam(b[c], g_b[c]) in place for c < n_components; the padding columns
 *                              of b and g_out are written as zeros.  b: [ld] fp32.
 *   tmf_adam_bias_rows_f32     one sweep over every row: W[i] = fresh-Adam(W[i], G[i]) in place (the arithmetic of
 *                              tmf_adam_fresh_rows_f32), then E[i] = W[i] + b_new.  Columns >= n_components of W and E are written
 *                              as zeros whatever W, G and b_new hold there.  W, G, E: [n_rows, ld], 16-byte aligned, W != E. */
int64_t tmf_bias_colsum_part_rows(int64_t n_rows);
int tmf_bias_colsum_f32(const float* G, int64_t n_rows, int n_components, double* part, int64_t part_rows, double* colsum,
                        void* stream);
int tmf_bias_adam_f32(const double* part, int64_t part_rows, float* b, float* g_out, int n_components, tmf_adam adam,
                      void* stream);
int tmf_adam_bias_rows_f32(float* W, const float* G, const float* b_new, float* E, int64_t n_rows, int n_components,
                           tmf_adam adam, void* stream);

/* LinearEmbedding over a SPARSE feature matrix F [rows, n_features] (embedding_graphs.py:30-38, features @ weights): the
 * effective table is E = F W.  The passes read E and, under TMF_EPI_GRAD, write G = dL/dE [rows, ld]; dL/dW = F^T G, and W takes the
 * fresh-Adam step (matrix_factorization.py:173-176).  Both products are one pass over a list view of F (tmf_segments over its
 * CSR lists, id = feature of every entry, or over its CSC lists, id = row of every entry; val = the entry's value beside it):
 *   g[i] = sum over the entries k of list row i of  val[k] * T[id[k]]   (no entry is skipped), then the epilogue:
 *   TMF_EPI_GRAD: X_out[i] = g[i] (fp32; X_old unused, may be NULL)      - E = F W over the CSR lists
 *   TMF_EPI_ADAM: X_out[i] = fresh_adam(X_old[i], g[i])                  - W step from G over the CSC lists
 * Rows of several segments go to `slab` and are finished by tmf_combine_rows_f32 with the same epi.
 * Tables are [rows, ld] fp32 with zero padding columns; an empty list row gives g = 0 (E row 0 / W row unchanged).
 * No atomics and a fixed order of additions: results are bit-identical from call to call.  id, val and T are only read.
 * Null tables or a bad epi: TMF_E_INVALID; nseg == 0: TMF_OK; nothing is launched in either case. */
int tmf_feat_pass_f32(const tmf_segments* seg, const int32_t* id, const float* val, const float* T,
                      const float* X_old, float* X_out, float* slab, int n_components, int epi, tmf_adam adam, void* stream);

/* ReLUEmbedding (embedding_graphs.py:61-87): E = relu(F Wr + b) W with the hidden width aux (5 r in the reference).  The sparse
 * products Z = F Wr and dWr = F^T dZ are tmf_feat_pass_f32 at width aux, the bias step is tmf_bias_colsum_f32 / tmf_bias_adam_f32
 * at width aux; these are the dense products in between, on the exact-fp32 MFMA.  Tables are fp32, 16-byte aligned:
 * Z, dZ [n_rows, ld(aux)], b [ld(aux)], W [aux, ld(r)], G, E [n_rows, ld(r)], ld = tmf_padded_ld.  The hidden value is
 * h = max(fl(z + b), 0) (one fp32 add) and a unit is on where fl(z + b) > 0, the same expression in every call; H is never
 * stored.  The padding columns of the inputs may hold anything; those of the outputs are written as zeros.
 *
 *   tmf_relu_embed_f32         E[i, c] = sum_a h[i, a] W[a, c].
 *   tmf_relu_dhidden_f32       dZ[i, a] = on(i, a) ? sum_c G[i, c] W[a, c] : 0 (exactly 0 where the unit is off).  dZ != Z.
 *   tmf_relu_part_rows         P, the blocks the rows are cut into for the weight gradient: a function of n_rows alone
 *                              (0 for n_rows <= 0, at most 256).
 *   tmf_relu_dweights_f32      part[p][a, c] = sum over the rows i of block p of h[i, a] G[i, c]; part: [P, aux, ld(r)] fp32.
 *   tmf_relu_adam_weights_f32  g = sum_p part[p] in the order p = 0, 1, .. (stored in g_out [aux, ld(r)] when it is not NULL), then
 *                              W_out = fresh_adam(W_old, g) (the arithmetic of tmf_adam_fresh_rows_f32).  part_rows = 0 (no rows):
 *                              g = 0 and W_out = W_old.
 * No atomics and a fixed order of additions: results are bit-identical from call to call.  Nothing is allocated; every call is
 * stream-ordered.  n_rows == 0: TMF_OK, nothing is launched.  A null table, aux or n_components outside [1, 1024], a table that
 * is not 16-byte aligned, dZ == Z or a part_rows other than tmf_relu_part_rows(n_rows): TMF_E_INVALID before anything is launched. */
int tmf_relu_embed_f32(const float* Z, const float* b, const float* W, float* E, int64_t n_rows, int aux, int n_components,
                       void* stream);
int tmf_relu_dhidden_f32(const float* G, const float* W, const float* Z, const float* b, float* dZ, int64_t n_rows, int aux,
                         int n_components, void* stream);
int64_t tmf_relu_part_rows(int64_t n_rows);
int tmf_relu_dweights_f32(const float* Z, const float* b, const float* G, float* part, int64_t part_rows, int64_t n_rows, int aux,
                          int n_components, void* stream);
int tmf_relu_adam_weights_f32(const float* part, int64_t part_rows, const float* W_old, float* W_out, float* g_out, int aux,
                              int n_components, tmf_adam adam, void* stream);

/* OPT-IN EXTENSION, not the reference's optimiser (which is rebuilt every epoch, matrix_factorization.py:176): Keras
 * Adam with persistent moments.  tmf_adam_step gives the scalars of iteration `step` (1-based; step 1 == tmf_adam_fresh),
 * tmf_adam_state_rows_f32 applies one step in place to a whole [n_rows, ld] table from its raw gradient G (the
 * TMF_EPI_GRAD output of the passes) and the moment tables M, V (zero before the first step). */
tmf_adam tmf_adam_step(float lr, int step);
int tmf_adam_state_rows_f32(float* W, const float* G, float* M, float* V, int64_t n_rows, int n_components,
                            tmf_adam adam, void* stream);

/* EXTENSION (the reference has no regularisation): L2-regularised twins of the four table steps.  The objective gains
 * alpha ||W||_F^2 per penalised table, so the raw gradient G of the data term (the TMF_EPI_GRAD output of the passes) becomes
 *   g' = fl(g + fl(l2 * w)),   l2 = 2 alpha (fp32), w the weight BEFORE the step
 * - one product and one sum, each rounded to nearest once, never contracted into an fma - and g' takes the op sequence of the
 * function extended, unchanged.  l2 = 0 gives that function's bits.  G is only read.
 *   tmf_adam_fresh_rows_l2_f32   W = fresh-Adam(W, g') in place over n_rows x ld floats (tmf_adam_fresh_rows_f32).
 *   tmf_adam_fresh_rows_l2_bf16  the same on a bf16-stored table: widened, stepped in fp32, rounded once; G fp32 [n_rows, ld],
 *                                ld = tmf_padded_ld_bf16 (tmf_adam_fresh_rows_bf16).
 *   tmf_adam_state_rows_l2_f32   tmf_adam_state_rows_f32 with g' for g: the moments M, V see g'.
 *   tmf_adam_bias_rows_l2_f32    tmf_adam_bias_rows_f32 with g' for g, w the raw weight W[i] (not E; the bias is never penalised);
 *                                columns >= n_components of W and E are written as zeros; W, G, b_new, E 16-byte aligned, W != E.
 * n_components outside [1, 1024], l2 negative or not finite (NaN included), a null table (n_rows > 0): TMF_E_INVALID and nothing
 * is launched; n_rows == 0: TMF_OK. */
int tmf_adam_fresh_rows_l2_f32(float* W, const float* G, int64_t n_rows, int n_components,
                               tmf_adam adam, float l2, void* stream);
int tmf_adam_fresh_rows_l2_bf16(void* W, const float* G, int64_t n_rows, int n_components,
                                tmf_adam adam, float l2, void* stream);
int tmf_adam_state_rows_l2_f32(float* W, const float* G, float* M, float* V, int64_t n_rows, int n_components,
                               tmf_adam adam, float l2, void* stream);
int tmf_adam_bias_rows_l2_f32(float* W, const float* G, const float* b_new, float* E, int64_t n_rows, int n_components,
                              tmf_adam adam, float l2, void* stream);

/* Deterministic sum of `n` floats into out[0] (fp64 accumulate, fixed order) - the reduce_mean
 * numerator of matrix_factorization.py:179. */
int tmf_sum_f32(const float* x, int64_t n, double* out, void* stream);

/* utils.py:94-105 gather_matrix_indices: out[i, c] = X[i, idx[i, c]];  X [rows, cols] fp32,
 * idx [rows, k] int64. */
int tmf_gather_rows_cols_f32(const float* X, const int64_t* idx, float* out, int64_t rows,
                             int64_t cols, int64_t k, void* stream);

/* K7: C[m, n] = A[m, :r] . B[n, :r]^T in exact fp32 on the f32 MFMA (matrix_factorization.py:149,195).
 * lda / ldb / ldc in floats. */
int tmf_predict_gemm_f32(const float* A, const float* B, float* C, int64_t m, int64_t n, int r,
                         int64_t lda, int64_t ldb, int64_t ldc, void* stream);

/* K8: row-wise top-k of X [rows, cols] ordered (value desc, index asc) - tf.math.top_k's contract
 * (matrix_factorization.py:245,429-438), any k in [1, cols] including the full ranking retrieve_user_recs(k=None) and
 * dcg / ndcg ask for (:336,:367,:424-438).  clamp_negatives != 0 first maps x <= 0 to 0.0 (matrix_factorization.py:237).
 * out_idx [rows, k] int32, out_val optional [rows, k].  k <= 64, or rows of at most 16384 columns, need no workspace;
 * larger k over wider rows is a stable segmented radix sort through `workspace` (tmf_topk_workspace_bytes; rows * cols
 * < 2^32 per call). */
size_t tmf_topk_workspace_bytes(int64_t rows, int64_t cols, int k);
int tmf_topk_stable_f32(const float* X, int64_t rows, int64_t cols, int64_t ldx, int k,
                        int clamp_negatives, int32_t* out_idx, float* out_val, void* workspace,
                        size_t workspace_bytes, void* stream);

/* bf16-storage / fp32-arithmetic variants (BASELINE config 5: "bf16 factors / fp32 accum"; an extension - the
 * reference is fp32 throughout).  Tables are bf16 row-major [rows, tmf_padded_ld_bf16(r)]; every product,
 * sum, loss and the optimiser step are computed in fp32 and the new row is rounded to bf16 once
 * (round-to-nearest-even).  slab / loss / delta / D / TMF_EPI_GRAD outputs stay fp32 (the raw gradient is what
 * RCCL reduce-scatters).  Arguments otherwise exactly as the _f32 functions. */
int tmf_mse_pass_bf16(const tmf_segments* seg, const int32_t* other, const float* val,
                      const void* X_old, const void* Y_old, void* X_out, float* slab,
                      float* loss_part, int n_components, int epi, tmf_adam adam, void* stream);
int tmf_kl_moments_bf16(const tmf_segments* seg, const int32_t* other, const float* val, const void* X_old,
                        const void* Y_old, double* part, int n_components, void* stream);
int tmf_kl_pass_bf16(const tmf_segments* seg, const int32_t* other, const float* val, const void* X_old,
                     const void* Y_old, void* X_out, float* slab, const double* coef, int n_components, int epi,
                     tmf_adam adam, void* stream);
int tmf_logistic_pass_bf16(const tmf_segments* seg, const int32_t* other, const float* val, const void* X_old,
                           const void* Y_old, void* X_out, float* slab, float* loss_part, int n_components, int epi,
                           tmf_adam adam, int weighted, void* stream);
int tmf_wsum_pass_bf16(const tmf_segments* seg, const int32_t* ent_row, const int32_t* ent_w,
                       const float* wbuf, const void* T, const void* X_old, void* X_out,
                       float* slab, int n_components, int epi, tmf_adam adam, void* stream);
int tmf_wsum_rows4_bf16(const int64_t* rowptr, int32_t n_rows, int32_t n_blocks, const int32_t* ent_row, const int32_t* ent_w,
                        const float* wbuf, const void* T, const void* X_old, void* X_out, int n_components, int epi,
                        tmf_adam adam, int32_t rows_per_launch, void* workspace, size_t workspace_bytes, void* stream);
int tmf_wsum_rows5_bf16(const int64_t* rowptr, int32_t n_rows, int32_t n_blocks, const int32_t* ent_row, const int32_t* ent_w,
                        const float* wbuf, const void* T, const void* X_old, void* X_out, float* slab, const int32_t* vr_item,
                        const int32_t* vr_part, const int32_t* vr_nparts, const int32_t* vr_slot, int32_t n_vrows, int n_components,
                        int epi, tmf_adam adam, int32_t rows_per_launch, void* workspace, size_t workspace_bytes, void* stream);
int tmf_combine_rows_bf16(const int32_t* long_rows, const int64_t* slab_beg, int64_t n_long,
                          const float* slab, const void* X_old, void* X_out, int n_components,
                          int epi, tmf_adam adam, void* stream);
int tmf_wmrb_user_pass_bf16(const int64_t* rowptr, const int32_t* col, const float* val,
                            const int32_t* R, int32_t n_users, int32_t S, float c,
                            const void* U_old, const void* V_old, void* U_out, float* delta,
                            float* D, float* loss_part, float* pos_part,
                            int n_components, int epi, tmf_adam adam, void* stream);
int tmf_adam_fresh_rows_bf16(void* W, const float* G, int64_t n_rows, int n_components,
                             tmf_adam adam, void* stream);

/* K7+K8 fused: out_idx[u, :k] = top-k (value desc, index asc) of A[u, :r] . B[:, :r]^T over all n items,
 * without materialising the [m, n] scores (recall_at_k / retrieve_user_recs, matrix_factorization.py:236-248,
 * :424-438, at catalog sizes where the dense matrix does not fit).  Supports k <= 64 and r <= 256; returns
 * TMF_E_UNSUPPORTED otherwise (callers then score block-wise with tmf_predict_gemm_f32 + tmf_topk_stable_f32). */
int tmf_predict_topk_f32(const float* A, const float* B, int64_t m, int64_t n, int r, int64_t lda,
                         int64_t ldb, int k, int clamp_negatives, int32_t* out_idx, float* out_val,
                         void* stream);

/* The same for bf16-stored tables (A [m, lda], B [n, ldb] bf16, ld %% 8 == 0) on the bf16 MFMA: products of
 * bf16 values are exact and accumulate in fp32 ("bf16 factors / fp32 accum").  k <= 32, r <= 256. */
int tmf_predict_topk_bf16(const void* A, const void* B, int64_t m, int64_t n, int r, int64_t lda,
                          int64_t ldb, int k, int clamp_negatives, int32_t* out_idx, float* out_val,
                          void* stream);

/* tmf_predict_topk_f32 for fp32 tables on the bf16 matrix cores, fp32-accurate: every factor is split exactly into three
 * bf16 planes and a score is the sum of the six plane products that weigh >= 2^-24 of the leading one, small ones first,
 * accumulated in fp32 (csrc/tmf_predict_split.hip; errors against fp64 at or below those of the fp32 MFMA kernel).  Same
 * outputs, order and tie rule as tmf_predict_topk_f32; values may differ from it by fp32 rounding.  r <= 256 (since version 203; 128 before), k <= 40 (32 before the 4-wave
 * instances of round 5: ask tmf_predict_topk_split_supported); `workspace` holds the item table's planes (query the size; overwritten per call). */
int tmf_predict_topk_split_supported(int r, int k);
size_t tmf_predict_topk_split_workspace_bytes(int64_t n, int r);
int tmf_predict_topk_split_f32(const float* A, const float* B, int64_t m, int64_t n, int r, int64_t lda,
                               int64_t ldb, int k, int clamp_negatives, int32_t* out_idx, float* out_val,
                               void* workspace, size_t workspace_bytes, void* stream);
/* The same ranking with TWO fp16 planes per factor and three plane products (h2 v1 + h1 v2 + h1 v1, fp32 accumulate): every
 * user row is scaled by its own power of two and the item table by one, so that the planes sit in fp16's normal range; 22
 * bits of every factor take part (all 24 with the three bf16 planes above), and a factor below ~1e-6 of its table's largest
 * magnitude keeps fewer.  Values against fp64: at the fp32 MFMA kernel's error (csrc/tmf_predict_split.hip, tests).  Half the
 * matrix-core work of the three-plane form.  r <= 256, k <= 32 (tmf_predict_topk_half2_supported); its own workspace size. */
int tmf_predict_topk_half2_supported(int r, int k);
size_t tmf_predict_topk_half2_workspace_bytes(int64_t n, int r);
int tmf_predict_topk_half2_f32(const float* A, const float* B, int64_t m, int64_t n, int r, int64_t lda,
                               int64_t ldb, int k, int clamp_negatives, int32_t* out_idx, float* out_val,
                               void* workspace, size_t workspace_bytes, void* stream);

/* Exclusion of already-seen (user, item) pairs from the rankings below ("rank what the user has not seen").  Row u's excluded
 * GLOBAL item ids are cols[rowptr[u] .. rowptr[u+1]), ascending (duplicates allowed); item_base is the global id of B's row 0
 * (X's column 0), so a window or shard of the catalog passes the same CSR with its own offset, and a block of users passes
 * rowptr + first_user.  Ids outside [item_base, item_base + n) are ignored.  Ordering, clamp and tie rule are those of the calls
 * without exclusion; a user with fewer than k eligible items gets id -1 (value -inf) in the trailing slots. */
typedef struct tmf_exclusion {
    const int64_t* rowptr;   /* [m + 1] device pointer */
    const int32_t* cols;     /* [rowptr[m]] device pointer */
    int64_t item_base;
} tmf_exclusion;

/* tmf_predict_topk_f32 / _bf16 / _split_f32 / _half2_f32 without the excluded pairs: an excluded score is removed before it
 * can become a candidate or raise a row's threshold.  Limits and workspaces as the plain calls. */
int tmf_predict_topk_exclude_f32(const float* A, const float* B, int64_t m, int64_t n, int r, int64_t lda,
                                 int64_t ldb, int k, int clamp_negatives, const tmf_exclusion* exclude,
                                 int32_t* out_idx, float* out_val, void* stream);
int tmf_predict_topk_exclude_bf16(const void* A, const void* B, int64_t m, int64_t n, int r, int64_t lda,
                                  int64_t ldb, int k, int clamp_negatives, const tmf_exclusion* exclude,
                                  int32_t* out_idx, float* out_val, void* stream);
int tmf_predict_topk_split_exclude_f32(const float* A, const float* B, int64_t m, int64_t n, int r, int64_t lda,
                                       int64_t ldb, int k, int clamp_negatives, const tmf_exclusion* exclude,
                                       int32_t* out_idx, float* out_val, void* workspace, size_t workspace_bytes, void* stream);
int tmf_predict_topk_half2_exclude_f32(const float* A, const float* B, int64_t m, int64_t n, int r, int64_t lda,
                                       int64_t ldb, int k, int clamp_negatives, const tmf_exclusion* exclude,
                                       int32_t* out_idx, float* out_val, void* workspace, size_t workspace_bytes, void* stream);
/* tmf_topk_stable_f32 without the excluded pairs (the non-fused path: k > 64, r > 256, full rankings).  X is OVERWRITTEN: the
 * clamp is applied to it in place and excluded entries become -inf; the workspace is tmf_topk_workspace_bytes(rows, cols, k).
 * An eligible score of -inf (an overflowing dot product) may be ranked behind excluded ones. */
int tmf_topk_stable_exclude_f32(float* X, int64_t rows, int64_t cols, int64_t ldx, int k, int clamp_negatives,
                                const tmf_exclusion* exclude, int32_t* out_idx, float* out_val, void* workspace,
                                size_t workspace_bytes, void* stream);

/* Full-catalog ranks of held-out (user, item) pairs (LightFM's predict_rank; auc_score and reciprocal_rank reduce them).
 * rank(u, i) = the number of ELIGIBLE items j != i - not excluded; other positives count - that the order of the fused top-k
 * (value desc, index asc) puts before i, so rank 0 is the top and, under the same arithmetic and exclusion, rank(u, i) < k holds
 * exactly when i is in the top-k list of u.  Scores are the raw u.v (no clamp); an item whose score is NaN is never counted above
 * anyone, and a positive whose own score is NaN ranks behind every non-NaN eligible item.
 *
 * The positives are addressed through VIRTUAL rows: a user with P positives is ceil(P / TMF_RANK_ROW_PAIRS) rows, each with at
 * most TMF_RANK_ROW_PAIRS of them; pos_item[begin[v] .. begin[v] + count[v]) are the (distinct) items of row v, user[v] its user
 * (rows of one user in any order; users without positives need no row).  Ranks are written to out_rank at the positives' own
 * positions.  A pair that is also excluded is the caller's error (its rank is undefined). */
#define TMF_RANK_ROW_PAIRS 16
typedef struct tmf_rank_rows {
    const int32_t* user;    /* [n_rows] */
    const int64_t* begin;   /* [n_rows] */
    const int32_t* count;   /* [n_rows], 1 .. TMF_RANK_ROW_PAIRS */
    int64_t n_rows;
} tmf_rank_rows;

/* out[p] = <A[pair_user[p]], B[pair_item[p]]> computed exactly as the fused rank kernel's tile computes it: _f32 on the fp32 MFMA
 * (as tmf_predict_topk_f32 / tmf_item_ranks_f32), _split on the three bf16 planes (as tmf_predict_topk_split_f32 /
 * tmf_item_ranks_split).  r <= 256 (TMF_E_UNSUPPORTED above for _split); tables as the top-k calls. */
int tmf_pair_scores_f32(const float* A, const float* B, int r, int64_t lda, int64_t ldb, const int32_t* pair_user,
                        const int32_t* pair_item, int64_t n_pairs, float* out, void* stream);
int tmf_pair_scores_split(const float* A, const float* B, int r, int64_t lda, int64_t ldb, const int32_t* pair_user,
                          const int32_t* pair_item, int64_t n_pairs, float* out, void* stream);

/* Fused GEMM + rank count over all n items, no [m, n] scores: pos_score = the pairs' scores from tmf_pair_scores_* of the SAME
 * form, exclude = NULL or the pairs to leave out (rows = users, ids as tmf_exclusion).  _f32: the fp32 MFMA arithmetic of
 * tmf_predict_topk_f32; _split: the three bf16 planes of tmf_predict_topk_split_f32, `workspace` holds the item planes
 * (tmf_item_ranks_split_workspace_bytes; overwritten per call).  r <= 256 (the _supported queries), TMF_E_UNSUPPORTED otherwise. */
int tmf_item_ranks_f32_supported(int r);
int tmf_item_ranks_split_supported(int r);
size_t tmf_item_ranks_split_workspace_bytes(int64_t n, int r);
int tmf_item_ranks_f32(const float* A, const float* B, int64_t n, int r, int64_t lda, int64_t ldb, const tmf_rank_rows* rows,
                       const int32_t* pos_item, const float* pos_score, const tmf_exclusion* exclude, int32_t* out_rank,
                       void* stream);
int tmf_item_ranks_split(const float* A, const float* B, int64_t n, int r, int64_t lda, int64_t ldb, const tmf_rank_rows* rows,
                         const int32_t* pos_item, const float* pos_score, const tmf_exclusion* exclude, int32_t* out_rank,
                         void* workspace, size_t workspace_bytes, void* stream);

/* The non-fused count (r > 256, bf16 tables, any arithmetic whose scores tmf_predict_gemm_f32 gives): X [rows, cols] holds the scores
 * of users [user_base, user_base + rows); `vrows` are the virtual rows of those users only.  With `exclude` (rows = global user ids)
 * the excluded entries of X are OVERWRITTEN with NaN first.  A positive's score is read from X. */
int tmf_rank_count_rows_f32(float* X, int64_t rows, int64_t cols, int64_t ldx, int64_t user_base, const tmf_rank_rows* vrows,
                            const int32_t* pos_item, const tmf_exclusion* exclude, int32_t* out_rank, void* stream);

/* DCG@k and IDCG@k of a graded test table (matrix_factorization.py:320-413) without the [m, n] scores.  Row u of the table is
 * cols / gain [rowptr[u] .. rowptr[u+1]): distinct item ids ascending and their gains (2^a - 1); every other eligible item has gain 0.
 *   dcg[u]  = sum_{j < k} gain(u, top[u * ldt + j]) / den[j]   (top: the user's ranked list, -1 = an empty slot; NULL without dcg)
 *   idcg[u] = sum_{j < k} g_(j) / den[j] over the k largest values of {the row's gains} + n_zero[u] zeros (fewer slots when the
 *             multiset is smaller); n_zero NULL = n_items - stored.
 * den [k]: the discount of every slot.  Sums run over the slots in order, slot 0 first (deterministic; no atomics).  dcg or idcg may
 * be NULL.  Any k >= 1; a row of any length (long rows are radix-selected by a workgroup, never sorted whole). */
int tmf_dcg_idcg_f32(const int64_t* rowptr, const int32_t* cols, const float* gain, int64_t m, int64_t n_items, const int32_t* top,
                     int64_t ldt, int k, const float* den, const int64_t* n_zero, float* dcg, float* idcg, void* stream);

/* EXTENSION (the reference ranks user-item scores only): unit rows for cosine similarity inside one side (similar_items /
 * similar_users rank them with the fused top-k).  Gather and normalisation in one launch, every source row read once:
 *   out[j, :r] = T[row_j, :r] / ||T[row_j, :r]||_2 as fp32,  norms[j] = that Euclidean norm (norms may be NULL),
 *   row_j = ids[j], or j when ids == NULL (then q <= n_rows).  ids may repeat and come in any order; the caller has checked
 *   them against [0, n_rows) - the library cannot (they are device memory).
 * T: fp32 (_f32) or bf16 (_bf16) rows of 16 bytes alignment - T 16-byte aligned, ldt %% 4 == 0 (bf16: ldt %% 8 == 0), ldt >= r;
 * only columns [0, r) of the rows asked for are read, so padding columns, skipped rows and other rows may hold anything.
 * out: fp32 [q, ldo], 16-byte aligned, ldo >= r, ldo %% 4 == 0; columns [0, ldo) of rows [0, q) are written, zeros in [r, ldo),
 * and nothing else is.  r in [1, 1024].
 * Arithmetic, right for every FINITE row whatever its scale: the row is multiplied by the power of two that brings its largest
 * magnitude into [1, 2) (exact), the squares are summed in fp32 in a fixed order (no atomics), square root and division are
 * correctly rounded, and the norm is scaled back by the same power of two (exact unless it leaves the fp32 range).  A row of
 * zeros gives a row of zeros and norm 0.  A row with a non-finite element is outside the contract (its outputs are unspecified).
 * The unit row depends on the row's contents and r alone: bit-identical wherever the row stands and whichever j asks for it.
 * q == 0: TMF_OK without a launch.  r, ldt, ldo, q, n_rows out of range, a null or misaligned table: TMF_E_INVALID before any
 * launch. */
int tmf_unit_rows_f32(const float* T, int64_t n_rows, int r, int64_t ldt, const int32_t* ids, int64_t q, float* out,
                      int64_t ldo, float* norms, void* stream);
int tmf_unit_rows_bf16(const void* T, int64_t n_rows, int r, int64_t ldt, const int32_t* ids, int64_t q, float* out,
                       int64_t ldo, float* norms, void* stream);

/* EXTENSION (the reference trains by gradient steps only): alternating least squares - implicit feedback after Hu, Koren and
 * Volinsky, and plain least squares over the stored entries.  fit_als / fold_in_users / fold_in_items are built on these entry
 * points.  TMF_VERSION stays 203, as for the other entry points added since: nothing that existed changes.
 *
 * G = T^T T, [r, r] fp32 (G[i * ldg + j]), r in [1, 128].  Blocks of rows give partial sums, which are added in block order: no
 * atomics, so reruns are bit-identical, and G is exactly symmetric.  Only columns [0, r) of T are read.  T 16-byte aligned,
 * ldt >= r, ldt %% 4 == 0, ldg >= r; `workspace` holds the partials (tmf_gram_workspace_bytes; overwritten per call).  n_rows == 0
 * gives zeros.  Anything out of range: TMF_E_INVALID before any launch. */
size_t tmf_gram_workspace_bytes(int64_t n_rows, int r);
int tmf_gram_f32(const float* T, int64_t n_rows, int r, int64_t ldt, float* G, int64_t ldg, void* workspace, size_t workspace_bytes,
                 void* stream);
/* The same contract for r in [1, 256] (the width the conjugate-gradient form takes); tmf_gram_f32 keeps its range and its bits. */
size_t tmf_gram_wide_workspace_bytes(int64_t n_rows, int r);
int tmf_gram_wide_f32(const float* T, int64_t n_rows, int r, int64_t ldt, float* G, int64_t ldg, void* workspace,
                      size_t workspace_bytes, void* stream);

/* One ALS half-step for q rows of a CSR (rowptr int64, col int32: ids of rows of Y; w, t: per-entry weight and target).  Row
 * `row` = ids[p], or p when ids == NULL, p < q, gets the solution of
 *     A x = b,   A = G0 + reg I + sum_k w[k] y_k y_k^T,   b = sum_k t[k] y_k,   y_k = Y[col[k], :r],  k in [rowptr[row], rowptr[row+1])
 * written to X[row * ldx ...]: columns [0, r) the solution, columns [r, ldx) exactly zero, and nothing else is written - with ids,
 * X is the whole table and rows not named keep their contents (a row named twice is written twice with the same bits).  G0: [r, r]
 * with pitch ldg (its lower triangle is read), or NULL for none.  A row without entries gets x = 0.  Duplicate columns add up.
 * Only columns [0, r) of the gathered rows of Y are read: padding columns and rows no entry names may hold anything.
 * Arithmetic: fp32 throughout; every sum over entries runs in entry order (the normal matrix on the fp32 MFMA, an fmaf chain) and
 * every step of the Cholesky factorisation A = L L^T and of the two triangular solves in a fixed order inside the one workgroup
 * that owns the row, so a row's x depends on its entries, Y, G0 and reg alone: bit-identical whichever launch, position in ids or
 * rerun computes it.  With reg > 0 and w >= 0, A is positive definite.  A pivot that is not a positive finite number fails the row:
 * its x is zeros and *n_failed (int32, device memory, zeroed by the caller) is incremented by an atomic add; no other row is affected.
 * r in [1, 128]; reg finite and > 0; Y and X 16-byte aligned, ldy >= r, ldy %% 4 == 0, ldx >= r, ldg >= r with G0: otherwise
 * TMF_E_INVALID before any launch.  q == 0: TMF_OK without a launch.  ids, col and rowptr are the caller's to check (device memory).
 * All row and entry offsets are 64-bit.
 * KNOWN LIMIT: one workgroup walks a row's entries serially, so a row with millions of entries serialises its workgroup; splitting
 * such rows into partial normal matrices is a follow-up.  Wider models take the conjugate-gradient form below. */
int tmf_als_solve_rows_f32(const float* Y, int64_t n_other, int r, int64_t ldy, const float* G0, int64_t ldg, const int64_t* rowptr,
                           const int32_t* col, const float* w, const float* t, float reg, const int32_t* ids, int64_t q, float* X,
                           int64_t ldx, int32_t* n_failed, void* stream);

/* The same half-step by cg_steps steps of conjugate gradients per row, r in [1, 256], cg_steps in [1, 32]; A is never formed
 * (A v = G0 v + reg v + sum_k w[k] (y_k . v) y_k).  teamoflow_amd/_als.py states the iteration: x starts from X0[row * ldx0 ...]
 * (X0 == NULL: zeros), stops early once res . res <= max(1e-14 b . b, 1e-30), and a row whose p . A p is not a positive finite
 * number fails as above (x = 0, *n_failed += 1).  A row without entries gets x = 0 whatever X0 held.
 * X0 == X with ldx0 == ldx (in place) is legal iff ids names no row twice - the caller's duty; otherwise X0 and X must not overlap.
 * Everything else as tmf_als_solve_rows_f32: columns [0, r) of a named row get the result and [r, ldx) exactly zero, rows not named
 * are untouched, only columns [0, r) of the gathered rows of Y and of the rows of X0 are read, only the lower triangle of G0 is read.
 * Arithmetic: fp32, every sum in a fixed order that depends on the row alone - 32 rows share a workgroup and the fp32 MFMA that
 * applies G0, but a row's x is a function of its entries, Y, G0, reg, its x0 and cg_steps only: bit-identical whichever launch,
 * position in ids or neighbours in the batch.
 * Y, X and X0 16-byte aligned; ldy, ldx (and ldx0 with X0) >= r and multiples of 4; ldg >= r with G0; reg finite and > 0: otherwise
 * TMF_E_INVALID before any launch.  q == 0: TMF_OK without a launch.
 * KNOWN LIMIT: a row of 1024 entries or more is walked by its whole workgroup, one such row at a time and once per application of
 * A (cg_steps + 1 times), so a row with millions of entries still serialises that workgroup. */
int tmf_als_cg_rows_f32(const float* Y, int64_t n_other, int r, int64_t ldy, const float* G0, int64_t ldg, const int64_t* rowptr,
                        const int32_t* col, const float* w, const float* t, float reg, const int32_t* ids, int64_t q, const float* X0,
                        int64_t ldx0, float* X, int64_t ldx, int cg_steps, int32_t* n_failed, void* stream);

/* EXTENSION (the reference draws its negative table once, on the host): the table of a resampling fit, drawn on the device in one
 * launch.  TMF_VERSION stays 203: nothing that existed changes.
 *
 * R[i, :] (int32 [n_users, n_samples], row-major, every element written and nothing else) = n_samples DISTINCT items of
 * [0, n_items) in random order for user u = user_offset + i: a function of (seed, u) alone, so blocks of users drawn by separate
 * calls are the rows of one table, and a second call gives the same bits.  It is exactly the table
 * teamoflow_amd/mf/utils.py random_sampler_device draws on its rejection branch, which is the definition:
 *   hash(a, b, c) = mix(mix(mix(a + (2 seed + 1) * 0x9E3779B97F4A7C15) ^ (b * 0xD6E8FEB86659FD93 + 0xA0761D6478BD642F))
 *                       ^ (c * 0xE7037ED1A0B428DB + 0x8EBC6AF09C88C6E3)),   mix = splitmix64's finaliser, all 64-bit wrapping;
 *   below(h) = (h >> 11) mod n_items  (logical shift: a 53-bit value);
 *   row[pos] = below(hash(u, pos, 2)), sorted ascending; then for rnd = 3 .. 66, while the row holds an element equal to its left
 *   neighbour: each such element, at place pos of the sorted row, becomes below(hash(u, pos, rnd)), and the row is sorted again;
 *   R[i, j] = row[ord[j]], ord = the places pos < n_samples ordered by (hash(u, pos, 0) >> 1, pos) ascending.
 * A row that still holds a repeat when round 66 begins stores a non-zero value to *failed (int32, device memory, zeroed by the
 * caller; a plain store, no atomic) - at 2 n_samples == n_items, the hardest case, rows settle within about 20 rounds.
 * tmf_sample_rows_supported: 1 <= n_samples <= 4096 (the row is sorted in LDS) and 2 n_samples <= n_items; the call returns
 * TMF_E_INVALID before any launch otherwise, for n_users < 0, user_offset < 0 or a null pointer.  n_users == 0: TMF_OK, no launch. */
int tmf_sample_rows_supported(int32_t n_items, int32_t n_samples);
int tmf_sample_rows(int32_t n_items, int64_t n_users, int32_t n_samples, int64_t seed, int64_t user_offset, int32_t* R,
                    int32_t* failed, void* stream);

/* EXTENSION (the reference's table is uniform): the table of tmf_sample_rows with every draw WEIGHTED - item i with probability
 * q_i / T - for popularity-weighted negatives (csrc/tmf_sample_weighted.hip).  TMF_VERSION stays 203: nothing that existed changes.
 *
 * cum: int64 [n_items], device memory, the inclusive prefix sum of integer weights q_i >= 0; T = cum[n_items - 1], 1 <= T < 2^33.
 * R[i, :] (int32 [n_users, n_samples], row-major, every element written and nothing else) = n_samples DISTINCT items of non-zero
 * weight in random order for user u = user_offset + i: a function of (seed, u, q) alone.  It is exactly the table
 * teamoflow_amd/mf/utils.py random_sampler_device(weights=q) draws, which is the definition - tmf_sample_rows's program with
 *   below(h) replaced by item(h) = the first i with cum[i] > (h >> 11) mod T   (an item of weight 0 is never drawn),
 *   and redraw rounds rnd = 3 .. 258.
 * A row that still holds a repeat when round 259 begins stores a non-zero value to *failed (int32, device memory, zeroed by the
 * caller; a plain store, no atomic).  The CALLER admits the weights: with H the sum of the n_samples largest q_i, 4 H <= 3 T - then a
 * redraw leaves the items of the row with probability >= 1/4, and the flag is set with probability <= 0.75^256 per place.  The
 * call does not check the rule, nor that cum ascends: whatever cum holds, every id written lies in [0, n_items) and the call ends.
 * tmf_sample_rows_weighted_supported: 1 <= n_samples <= 4096 (the row is sorted in LDS) and n_items >= 1; the call returns
 * TMF_E_INVALID before any launch otherwise, for n_users < 0, user_offset < 0, a null pointer, or cum[n_items - 1] outside
 * [1, 2^33) - the host reads that one word in stream order and waits for it (so the call cannot be captured into a graph) and hands
 * it to the kernel, which does not read it again.  n_users == 0: TMF_OK, no launch and nothing read. */
int tmf_sample_rows_weighted_supported(int32_t n_items, int32_t n_samples);
int tmf_sample_rows_weighted(const int64_t* cum, int32_t n_items, int64_t n_users, int32_t n_samples, int64_t seed,
                             int64_t user_offset, int32_t* R, int32_t* failed, void* stream);

/* EXTENSION (the reference has no softmax): the softmax of a positive against the WHOLE catalog - FullSoftmaxLoss - without the
 * [m, n] score matrix (csrc/tmf_fullsoftmax.hip).  TMF_VERSION stays 203: nothing that existed changes.
 * All three take fp32 tables of 1 <= n_components <= tmf_fsm_max_components (128) - any value, not only multiples of 4 - on
 * v_mfma_f32_32x32x2_f32; beyond it they return TMF_E_UNSUPPORTED before any launch.  A, B: [rows, ld] row-major, 16-byte aligned,
 * ld % 4 == 0, ld >= n_components; columns >= n_components are never used, whatever they hold.  No atomics: every output is
 * bit-identical from run to run.
 *
 *   tmf_fsm_lse_f32   lse[u] = log sum_{i < n} exp(A[u] . B[i]) for u < m, by a running maximum: finite for every finite score.
 *                     A row of A that holds a NaN (or whose scores reach +inf) gets a non-finite lse; no other row reads it.
 *                     lse: [m] fp32; nothing beyond lse[m - 1] is written.  m == 0: TMF_OK, no launch.
 *   tmf_fsm_wsum_f32  G[a, c] += sum_{b < nb} w_u exp(A[a] . B[b] - lse_u) B[b, c]   for a < ma, c < n_components,
 *                     where u, the row lse and w are indexed by, is a when user_is_a == 1 (lse, w: [ma]) and b when user_is_a == 0
 *                     (lse, w: [nb]).  `+=`: the sums are added onto what G [ma, ldg] holds, one read and one write per element;
 *                     columns >= n_components of G are not touched.  user_is_a == 1: a row with w[a] == 0 is not written at all.
 *                     user_is_a == 0: a swept row with w[b] == 0 contributes nothing, whatever lse[b] is.  ma == 0 or nb == 0:
 *                     TMF_OK, no launch.
 *   tmf_fsm_pos_pass_f32  the arguments of tmf_mse_pass_f32 up to the slab, always under TMF_EPI_GRAD: G_out[row] = - sum of
 *                     Y_old[other[k]] over the entries k of the row with val[k] > 0 (zeros for a row without one; a NaN value is not
 *                     > 0); rows cut into several segments leave their parts in the slab for tmf_combine_rows_f32, as there.
 *                     loss_part != NULL (then lse != NULL, [table rows]): loss_part[seg] = sum over those entries of
 *                     (lse[row] - X_old[row] . Y_old[other[k]]), for tmf_sum_f32. */
int tmf_fsm_max_components(void);
int tmf_fsm_lse_f32(const float* A, const float* B, int64_t m, int64_t n, int n_components, int64_t lda, int64_t ldb, float* lse,
                    void* stream);
int tmf_fsm_wsum_f32(const float* A, const float* B, int64_t ma, int64_t nb, int n_components, int64_t lda, int64_t ldb,
                     const float* lse, const float* w, int user_is_a, float* G, int64_t ldg, void* stream);
int tmf_fsm_pos_pass_f32(const tmf_segments* seg, const int32_t* other, const float* val, const float* X_old, const float* Y_old,
                         float* G_out, float* slab, const float* lse, float* loss_part, int n_components, void* stream);

/* EXTENSION (the reference's scores have no item term): the scalar item bias of the table family - scores U[u] . V[i] + b[i] - as two
 * passes around the pair step of the sliced user pass (csrc/tmf_itembias.hip).  Neither reads a factor table.  TMF_VERSION stays 203:
 * nothing that existed changes.  No atomics and a fixed order of additions: every output is bit-identical from call to call and does
 * not depend on the grid.  Nothing is allocated; both are stream-ordered and graph-capturable.
 *
 *   tmf_item_bias_add   sp[u, s] += b[R[u, s]] for u < n_users, s < n_samples and pk[k] += b[col[k]] for k < nnz: one fp32 add per
 *                       score, so a non-finite b[i] reaches the scores of item i only.  b: [n_items] fp32; R, sp: [n_users, n_samples]
 *                       contiguous (16-byte pieces where both are 16-byte aligned, element by element otherwise and behind the last
 *                       whole piece); col, pk: [nnz].  The ids are the plan's, already checked to lie in [0, n_items).  n_users = 0,
 *                       n_samples = 0 and nnz = 0 are TMF_OK (nothing to add: no launch when all scores are absent); a negative
 *                       count or a null pointer to something that is read: TMF_E_INVALID before any launch.
 *   tmf_item_bias_grad  g[i] = the sum of wbuf[ent_w[e]] over the entries e of the list rows blk * n_items + i, blk < user_chunks, of
 *                       rowptr_e [user_chunks * n_items + 1] (the WmrbPlan entry lists; what lies behind the last list row is never
 *                       read), then b_out[i] = fresh-Adam(b_old[i], g[i]) under TMF_EPI_ADAM (the arithmetic of tmf_adam_fresh_rows_f32)
 *                       or b_out[i] = g[i] under TMF_EPI_GRAD (b_old may be NULL).  b_out may be b_old.  A list row is cut into chunks
 *                       of `chunk` entries, every chunk summed by one wave in fp64: chunk 0 of every list row always, and the chunks
 *                       c >= 1 the caller lists - xrow[k] / xchunk[k] (list row, chunk) for k < n_extra, ordered by (item, block,
 *                       chunk), xptr [n_items + 1] the first k of every item - which must be all chunks c >= 1 that hold entries.
 *                       The chunk sums go to the workspace; item i adds chunk 0 of its blocks in block order, then its further
 *                       chunks in k order, and rounds to fp32 once.  An item without entries gets g = 0 exactly, and fresh-Adam
 *                       leaves its bias as it is.  n_extra = 0: xrow / xchunk / xptr are not read.  n_items = 0: TMF_OK.
 *   tmf_item_bias_grad_workspace_bytes  (user_chunks * n_items + n_extra) fp64 sums; the workspace is 8-byte aligned. */
int tmf_item_bias_add(const float* b, int32_t n_items, const int32_t* R, int64_t n_users, int32_t n_samples, float* sp,
                      const int32_t* col, int64_t nnz, float* pk, void* stream);
size_t tmf_item_bias_grad_workspace_bytes(int32_t n_items, int32_t user_chunks, int64_t n_extra);
int tmf_item_bias_grad(const int64_t* rowptr_e, int32_t n_items, int32_t user_chunks, const int32_t* ent_w, const float* wbuf,
                       int32_t chunk, const int32_t* xrow, const int32_t* xchunk, const int64_t* xptr, int64_t n_extra,
                       const float* b_old, float* b_out, int epi, tmf_adam adam, void* workspace, size_t workspace_bytes,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TMF_H */
