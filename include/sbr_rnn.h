/* sbr_rnn.h -- C-ABI of libsbr_rnn.so: the MI355X (gfx950) engine for the
 * `train.py -m RNN` training hot path of rdevooght/sequence-based-recommendations.
 *
 * The reference has no FFI for this path: its seam is three Theano-compiled callables
 * plus a parameter list, all owned by RNNBase (neural_networks/rnn_base.py):
 *     train_function(*theano_inputs) -> cost        built :185, called :290
 *     test_function(theano_inputs, k) -> ids[k]     built :196-211, called :361
 *     predict_function(X, mask) -> scores (1,N)     built :188-194, called :151
 *     lasagne.layers.get/set_all_param_values       :476, :515
 * Each entry point below cites the reference interface it replaces.  Plain pointers and
 * sizes only; no torch types.  All functions return 0 on success or a negative
 * sbr_status; sbr_last_error() gives the message (thread-local).  Nothing throws across
 * the ABI.  A handle is not thread-safe (one stream, one host thread per rank), which
 * matches the reference's single-threaded synchronous calls (rnn_base.py:285-300).
 *
 * Memory: the caller may hand in a device arena (e.g. a torch tensor's data_ptr(), so
 * that torch.distributed/RCCL can all-reduce the gradient section in place); with
 * arena == NULL the library hipMallocs its own.
 */
#ifndef SBR_RNN_H
#define SBR_RNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SBR_MAX_LAYERS 4
#define SBR_ABI_VERSION 11

typedef enum { SBR_OK = 0, SBR_EINVAL = -1, SBR_ENOMEM = -2, SBR_EHIP = -3, SBR_ESTATE = -4,
               SBR_EUNSUPPORTED = -5 } sbr_status;

/* --r_t (recurrent_layers.py:9) */
typedef enum { SBR_CELL_LSTM = 0, SBR_CELL_GRU = 1, SBR_CELL_VANILLA = 2 } sbr_cell;
/* --loss (command_parser.py:43, :116-121) */
typedef enum { SBR_LOSS_CCE = 0, SBR_LOSS_BLACKOUT = 1, SBR_LOSS_BPR = 2, SBR_LOSS_TOP1 = 3,
               /* RNNMargin (rnn_margin.py:62-69; command_parser.py:118-119): linear output layer, multi-target losses */
               SBR_LOSS_HINGE = 4, SBR_LOSS_LOGIT = 5, SBR_LOSS_LOGSIG = 6,
               /* RNNCluster's further sampled losses (rnn_cluster.py:158-175; `--clusters C` with --loss CCE | BPRelu | lin):
                * cross-entropy over the sampled columns, leaky hinge on the score differences, plain differences */
               SBR_LOSS_SCCE = 7, SBR_LOSS_BPRELU = 8, SBR_LOSS_LIN = 9 } sbr_loss;
#define SBR_LOSS_IS_MARGIN(l) ((l) >= SBR_LOSS_HINGE && (l) <= SBR_LOSS_LOGSIG)
/* --u_m (update_manager.py:4) */
typedef enum { SBR_UPD_ADAGRAD = 0, SBR_UPD_ADADELTA = 1, SBR_UPD_RMSPROP = 2, SBR_UPD_NESTEROV = 3,
               SBR_UPD_ADAM = 4 } sbr_updater;

/* Everything RNNBase.__init__/prepare_model fixes (rnn_base.py:61-109, rnn_one_hot.py:37-78,
 * rnn_sampling.py:93-137, recurrent_layers.py:18-26, update_manager.py:24-82). */
typedef struct sbr_config {
    int32_t abi_version;            /* SBR_ABI_VERSION */
    int32_t cell;                   /* sbr_cell */
    int32_t n_layers;               /* --r_l "100-50" -> 2 */
    int32_t layers[SBR_MAX_LAYERS]; /* hidden units per layer */
    int32_t n_items;                /* N: output units (data/stats, data_handling.py:94) */
    int32_t input_size;             /* rows of layer-0 W_in = N + n_optional_features (rnn_one_hot.py:48-49) */
    int32_t n_feat;                 /* F indices per step: 1, or 2 with --rf (rnn_base.py:615-642) */
    int32_t max_length;             /* T (--max_length) */
    int32_t batch_size;             /* global batch B: the mean in the cost (rnn_one_hot.py:71) */
    int32_t local_batch;            /* rows this rank holds per step (== batch_size on one GPU) */
    int32_t row_offset;             /* first global row of this rank (sampled heads: positive column) */
    int32_t loss;                   /* sbr_loss */
    int32_t n_samples;              /* S = effective_sampling (rnn_sampling.py:102-106); 0 for CCE */
    int32_t updater;                /* sbr_updater */
    float learning_rate;            /* --u_l */
    float rho;                      /* --u_rho (adadelta/rmsprop rho, nesterov momentum) */
    float beta1, beta2;             /* --u_b1 --u_b2 */
    float regularization;           /* -r: >0 L2, <0 L1, on b_out only (rnn_one_hot.py:73-77) */
    float grad_clip;                /* 100 (recurrent_layers.py:19); <=0 disables */
    int32_t flags;                  /* SBR_FLAG_* */
    int32_t embedding_size;         /* --r_emb E (recurrent_layers.py:46-50): EmbeddingLayer (input_size, E) + flatten in front of
                                     * DENSE recurrent layers (layer 0 input = n_feat * E); 0 = index-input layer 0 */
    int32_t bidirectional;          /* --r_bi (recurrent_layers.py:70-76): every level = a forward and a backwards layer over the same
                                     * input, concatenated on the feature axis (next level / output layer see 2*H features) */
    /* RNNMargin only (losses hinge / logit / logsig; rnn_margin.py:32-51, :112-147) */
    float balance;                  /* --balance: weight of a false positive = balance * n_pos / (N - n_pos - n_in) */
    int32_t n_targets;              /* --n_targets: positives per row at most (columns of `target` in sbr_set_batch, -1 = none) */
    int32_t unique;                 /* interactions_are_unique (not --repeated_interactions): a row's input items get weight 0, target 0 */
} sbr_config;

#define SBR_FLAG_SIMPLE_REC  1   /* triage: per-step VALU recurrent kernels instead of the MFMA persistent ones */
#define SBR_FLAG_SIMPLE_GEMM 2   /* triage: naive GEMM instead of the MFMA tiled one */
#define SBR_FLAG_F32_MFMA 16      /* recurrent GEMM on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32) instead of the bf16x6 split */
#define SBR_FLAG_PROFILE_REC 8    /* recurrent kernels record s_memtime / s_memrealtime phase counters ("prof" debug buffer) */
#define SBR_FLAG_ATOMIC_SCATTER 4 /* triage: per-element float atomics instead of the sorted segment reduce */
/* Row-sparse optimizer (see "Row-sparse blocks" below): by default a block is stepped row by row when a step cannot touch
 * every row of it anyway (more rows than the batch has item ids / more items than sampled cells). */
#define SBR_FLAG_SPARSE_UPDATE 32 /* always, for every block that exists (tests) */
#define SBR_FLAG_DENSE_UPDATE 64  /* never: one dense elementwise pass over every parameter, as lasagne.updates.* does */
/* Output projection h . W_out (DenseLayer rnn_one_hot.py:65 / BlackoutLayer's deterministic branch sparse_lstm.py:37-40) on
 * plain bf16 operands with f32 accumulation (one v_mfma_f32_16x16x32_bf16 per block): the training forward of the full
 * softmax and predict / top-k of every head.  Scores then carry bf16 input rounding (~3e-3 of their spread) instead of
 * float32 rounding; gradients still come from the float32-class kernels. */
#define SBR_FLAG_BF16_PROJECTION 128
/* The dense GEMMs between stacked recurrent layers (recurrent_layers.py:94-104: layer l >= 2 reads the hidden states of layer
 * l - 1 through a dense W_in; its backward pair dW_in = h^T . dxt and dh = dxt . W_in^T) on plain bf16 operands with f32
 * accumulation, one MFMA per product (BASELINE configs[4]: "bf16 MFMA output projection (and bf16 layer-2 input GEMM)").  Default:
 * the f32-class two-plane fp16 split (three MFMAs).  Gradients then carry bf16 input rounding (~4e-3 relative per product). */
#define SBR_FLAG_BF16_LAYERS 256

typedef struct sbr_handle sbr_handle;

const char* sbr_last_error(void);
int sbr_abi_version(void);

/* Bytes of device arena a handle for this config needs (params + grads + optimizer state +
 * activations saved for BPTT + workspaces). */
int sbr_arena_bytes(const sbr_config* cfg, size_t* bytes);

/* Replaces RNNBase.prepare_model + _compile_*_function (rnn_base.py:106-109, :175-213).
 * arena: device pointer of >= sbr_arena_bytes() bytes, 256-B aligned, or NULL (library
 * allocates).  stream: hipStream_t every launch goes to (NULL = default stream).
 * Parameters start as zeros: call sbr_set_params. */
int sbr_create(const sbr_config* cfg, void* arena, size_t arena_bytes, void* stream, sbr_handle** out);
void sbr_destroy(sbr_handle* h);

/* lasagne.layers.get_all_param_values / set_all_param_values (rnn_base.py:476, :515):
 * n arrays in Lasagne order and shape (float32, C-contiguous, host memory); LSTM layer:
 * 12 gate arrays, 3 peepholes, cell_init, hid_init; GRU: 9 gate arrays, hid_init; then
 * out.W (H,N), out.b (N,)  (sparse_lstm.py:240-279, :660-676). */
int sbr_num_params(const sbr_handle* h);
int sbr_param_shape(const sbr_handle* h, int i, int64_t dims[2], int* ndim);
/* Name and shape of array i of that list for a configuration -- host only, no device or handle needed (tooling: which
 * arrays are weights / biases / initial states, for the init laws of the Lasagne layers).  "l0.W_in_to_ingate", "emb.W",
 * "out.W" ...; a Vanilla layer with dense input is the stock RecurrentLayer and lists hid_init, input_to_hidden.W,
 * input_to_hidden.b, hidden_to_hidden.W (recurrent_layers.py:94-104).  i past the end: SBR_EINVAL. */
int sbr_describe_param(const sbr_config* cfg, int i, char* name, size_t name_cap, int64_t dims[2], int* ndim);
int sbr_set_params(sbr_handle* h, int n, const float* const* host_arrays);
int sbr_get_params(sbr_handle* h, int n, float* const* host_arrays);
/* Same layout, gradients of the last forward/backward (parity tests). */
int sbr_get_grads(sbr_handle* h, int n, float* const* host_arrays);

/* Flat device sections (float32).  The gradient section carries one extra trailing float:
 * the batch cost, so that one all-reduce sums gradients and cost across ranks.
 * which: 0 params, 1 grads(+cost), 2 optimizer state.  split_floats (grads only): offset of
 * the output-layer gradients, which are complete after sbr_loss_backward_output and can be
 * all-reduced while sbr_backward_recurrent runs. */
int sbr_section(sbr_handle* h, int which, void** dev_ptr, size_t* n_floats, size_t* split_floats);

/* RNNMargin, --pb: the default target of every item (RNNMargin._default_target, rnn_margin.py:149-161: min(1 - p_i,
 * (1 - min_access) p_i / min_access)), N floats on the host; without a call (or with NULL) it is 0 everywhere. */
int sbr_set_default_target(sbr_handle* h, const float* default_target);

/* The per-call inputs of train_function (rnn_one_hot.py:61,106; rnn_sampling.py:128,194):
 * X int32 (B,T,F) left-aligned; lengths int32 (B,) = mask.sum(1) (masks are prefix masks,
 * rnn_one_hot.py:100-101); target int32 (Bg,) -- all GLOBAL rows for the sampled heads
 * (Blackout's softmax spans every target, rnn_sampling.py:68-72,137), local rows for CCE;
 * samples int32 (S,) or NULL; target_popularity float (B,) local rows (pop**db,
 * rnn_one_hot.py:103).  `exclude` (B,N) is never materialised (unused by train_function,
 * rnn_base.py:185 on_unused_input='ignore').  on_device != 0: pointers are device memory. */
int sbr_set_batch(sbr_handle* h, const int32_t* X, const int32_t* lengths, const int32_t* target,
                  const int32_t* samples, const float* target_popularity, int n_rows, int on_device);

/* train_function(*batch) -> cost (rnn_base.py:290): zero grads, forward, loss, backward,
 * update.  cost_host may be NULL (cost stays on device: sbr_read_cost). */
int sbr_train_step(sbr_handle* h, float* cost_host);
/* The training loop's form of the same call (rnn_base.py:285-300 reads the cost of every iteration): enqueues the step
 * and a copy of its cost, and hands back the cost of the PREVIOUS call once that is ready, so the host never waits for
 * the step it has just enqueued.  *have_prev = 0 on the first call.  sbr_lagged_flush waits for and returns the cost of
 * the last enqueued step (call it before reading parameters, validating, or leaving the loop). */
int sbr_train_step_lagged(sbr_handle* h, float* prev_cost, int* have_prev);
int sbr_lagged_flush(sbr_handle* h, float* cost, int* have);
/* The same in phases (data-parallel: all-reduce the gradient section between them). */
int sbr_zero_grads(sbr_handle* h);
int sbr_forward(sbr_handle* h);
int sbr_loss_backward_output(sbr_handle* h);
int sbr_backward_recurrent(sbr_handle* h);
int sbr_apply_update(sbr_handle* h);
int sbr_read_cost(sbr_handle* h, float* cost_host);
/* The lagged cost for the phase-by-phase form: call it behind sbr_apply_update.  It enqueues the report of the cost word at the
 * end of the gradient section (after a data-parallel driver's all-reduce: the GLOBAL cost) and of the fault word on `stream`,
 * and hands back the report of the previous call -- sbr_read_cost without the wait for the stream.  Same slots and sequence
 * numbers as sbr_train_step_lagged, which is sbr_train_step + this call; sbr_lagged_flush serves both forms. */
int sbr_cost_lagged(sbr_handle* h, float* prev_cost, int* have_prev);
/* The phases put everything that only feeds the optimizer (output-layer weight/bias gradients, the cost, the
 * weight-gradient kernels) on an internal side stream.  Called one by one they join it at their end so that the
 * caller may read the gradients on `stream`.  A data-parallel driver that orders its collectives itself turns the
 * joins off: after sbr_loss_backward_output the output-layer slice is complete ON THE SIDE STREAM (sbr_query
 * "side_stream" returns it) -- all-reduce it from there while `stream` runs the BPTT chain -- and calls
 * sbr_join_side before touching the rest.  sbr_apply_update always joins. */
int sbr_set_deferred_join(sbr_handle* h, int on);
int sbr_join_side(sbr_handle* h);

/* ------------------------------------------------------------------------------------------------
 * Row-sparse blocks.  The reference's updates are dense over every parameter (update_manager.py:24-82, lasagne.updates.*);
 * only the rows a batch gathers (sparse_lstm.py:368) and the sampled cells (sparse_lstm.py:50-54) receive a non-zero
 * gradient.  Block kinds: the index-addressed rows of layer 0 (W_in of both directions, or the --r_emb table), and -- for
 * the sampled heads -- the rows of W_out / b_out.  A sparse block is stepped row by row over the touched rows only:
 * exact for adagrad (its zero-gradient step is a no-op); for rmsprop / adadelta / nesterov / adam the zero-gradient steps
 * a row missed are replayed when the row is next read or stepped ("lazy-exact": same results as the dense pass to
 * float32 rounding).  sbr_get_params, sbr_section(0 / 2), sbr_predict_scores and sbr_topk bring everything they read up to
 * date themselves; sbr_flush_lazy does it explicitly (e.g. before reading the parameter section through a pointer
 * obtained earlier). */
int sbr_flush_lazy(sbr_handle* h);
/* Data-parallel exchange of a sparse block b (0 .. sbr_query("sparse_blocks") - 1) instead of an all-reduce of the whole
 * block: after sbr_backward_recurrent,
 *   sbr_sparse_pack        moves this rank's touched gradient rows into ids_dev [max_local_rows] / rows_dev
 *                          [max_local_rows][row_floats] (device buffers of the caller, e.g. torch tensors handed to RCCL)
 *                          and returns their number (synchronises the stream);
 *   (the ranks all-gather ids and rows)
 *   sbr_sparse_unpack_add  adds ONE rank's rows into the gradient block; call it for every rank, own rows included, in
 *                          rank order on every rank, so that the replicas stay bit-identical;
 * sbr_apply_update then steps the union of the gathered rows.  sbr_dense_ranges lists the [lo, hi) float ranges of the
 * gradient section (trailing cost included) that still take the dense all-reduce. */
int sbr_sparse_info(sbr_handle* h, int b, int64_t* n_rows, int64_t* row_floats, int64_t* max_local_rows);
int sbr_sparse_pack(sbr_handle* h, int b, int32_t* ids_dev, float* rows_dev, int32_t* count_host);
int sbr_sparse_unpack_add(sbr_handle* h, int b, const int32_t* ids_dev, const float* rows_dev, int count);
int sbr_dense_ranges(sbr_handle* h, int cap, int64_t* lo, int64_t* hi, int* n);
/* The same exchange without a host round trip (ABI 7): the number of packed rows stays on the device and travels IN BAND.
 *   sbr_sparse_pack_device     ids_dev is [1 + max_local_rows] ints: ids_dev[0] = the row count, ids_dev[1 ..] the ids;
 *                              rows_dev [max_local_rows][row_floats].  Nothing is synchronised.
 *   (the ranks all-gather both buffers at their fixed capacity: ids_all [world][1 + max_local_rows], rows_all
 *    [world][max_local_rows][row_floats])
 *   sbr_sparse_unpack_add_all  adds every rank's rows in rank order (one launch per rank, its count read on the device).
 * A fixed-capacity all-gather moves max_local_rows rows per rank whatever the step touched: the caller chooses per block
 * between this form (small blocks: the host read is the cost) and the counted one above (large blocks: the bytes are). */
int sbr_sparse_pack_device(sbr_handle* h, int b, int32_t* ids_dev, float* rows_dev);
int sbr_sparse_unpack_add_all(sbr_handle* h, int b, const int32_t* ids_all, const float* rows_all, int world);

/* ------------------------------------------------------------------------------------------------
 * The cluster head of RNNCluster (`--clusters C`; rnn_cluster.py:237-256 the cluster loss, :275-300 its training and the hard
 * clusters, :327-352 the test function).  A second object beside the engine: it owns the cluster-selection weights Wc (H, C)
 * and the item / cluster repartition R (N, C), reads the user representation (the engine's final hidden state: device pointer,
 * row stride and the offset of the backwards half from sbr_debug_buffer("h_last")) and trains only its own two arrays, with its
 * own updater state and step count, as the reference's second `self.updater(...)` call does.  The recurrent network's sampled
 * head and loss are the engine's (losses SBR_LOSS_BLACKOUT .. SBR_LOSS_LIN).  Single rank (the head is not sharded). */
typedef enum { SBR_CLUSTER_MIX = 0, SBR_CLUSTER_SOFTMAX = 1, SBR_CLUSTER_SIGMOID = 2 } sbr_cluster_type;   /* --cluster_type */
typedef struct sbr_cluster_config {
    int32_t abi_version;            /* SBR_ABI_VERSION */
    int32_t n_items;                /* N */
    int32_t n_hidden;               /* H: features of the user representation (2 x the top layer's width with --r_bi) */
    int32_t hidden_split;           /* features [0, hidden_split) sit at columns [0, ..) of a row, the rest at off2 + (k - hidden_split) */
    int32_t n_clusters;             /* --clusters */
    int32_t cluster_type;           /* sbr_cluster_type */
    int32_t loss;                   /* sbr_loss: Blackout / BPR / TOP1 / SCCE (--loss CCE) / BPRelu / lin (rnn_cluster.py:88-101) */
    int32_t batch_size;             /* B rows per step: row b's positive is column b of the score matrix */
    int32_t max_samples;            /* most cluster samples per step (--c_sampling, or --sampling when unset) */
    int32_t updater;                /* sbr_updater */
    float learning_rate, rho, beta1, beta2;
    float scale;                    /* --init_scale (sbr_cluster_set_scale follows --scale_growing_rate) */
    float noise_std;                /* --csn: std of the gaussian noise on the selection activations in training (a counter-based
                                     * generator here, MRG_RandomStreams there: equal in law, not in stream) */
    uint64_t seed;
} sbr_cluster_config;
typedef struct sbr_cluster sbr_cluster;
sbr_cluster* sbr_cluster_create(const sbr_cluster_config* cfg, void* hip_stream);
void sbr_cluster_destroy(sbr_cluster* c);
int sbr_cluster_set_params(sbr_cluster* c, const float* R_host, const float* Wc_host);          /* [N][C], [H][C] */
int sbr_cluster_get_params(sbr_cluster* c, float* R_host, float* Wc_host);
int sbr_cluster_get_grads(sbr_cluster* c, float* dR_host, float* dWc_host);                      /* of the last forward_backward */
int sbr_cluster_set_scale(sbr_cluster* c, float scale);                                          /* T_scale.set_value, rnn_cluster.py:400 */
/* cost_clusters and its gradients for the B rows of h_dev (row stride ld_h floats) with targets_dev [B] and samples_dev
 * [n_samples]; cost_host may be NULL (nothing is synchronised then) */
int sbr_cluster_forward_backward(sbr_cluster* c, const float* h_dev, int ld_h, int off2, const int32_t* targets_dev,
                                 const int32_t* samples_dev, int n_samples, float* cost_host);
int sbr_cluster_apply_update(sbr_cluster* c);
/* test path: csel_dev[r] = argmax of the selection activations of row r (z_dev [rows][C] receives them when not NULL) */
int sbr_cluster_select(sbr_cluster* c, const float* h_dev, int ld_h, int off2, int rows, int32_t* csel_dev, float* z_dev);
/* scores_dev[r][n] *= hard[n][csel[r]] (NULL: skip), n_used_dev[r] = sum_n hard[n][csel[r]] (NULL: skip) */
int sbr_cluster_mask_scores(sbr_cluster* c, float* scores_dev, int ld, int rows, const int32_t* csel_dev, float* n_used_dev);
int sbr_cluster_hard(sbr_cluster* c, float* hard_host);                                          /* [N][C] = _get_hard_clusters() */
/* Ranking inside each row's item cluster on the device (added under ABI 11: two symbols, no struct change) -- the batched form of
 * RNNCluster.predict_function / top_k_recommendations (rnn_cluster.py:302-325, :461-487; test.py:61-76).
 * sbr_cluster_lists: the hard clusters of prepare_tests (rnn_cluster.py:440-466; NOT the f(100 R) of sbr_cluster_hard) as a CSR over
 * the clusters.  members(c) holds every item i with R[i][c] > 0, and every item without a positive entry whose fallback cluster is c:
 * the reference's scan (best = 0, best_val = R[i][0]; in order, only R[i][j] > best_val replaces it; NaN compares false).  Lists are
 * ascending in id; an item may sit in several, a list may be empty.  Built on the device from R on first use and kept until R changes
 * (sbr_cluster_set_params, sbr_cluster_apply_update).  sizes_host [C]; members_host NULL, or [sum of sizes]: list 0, list 1, ... */
int sbr_cluster_lists(sbr_cluster* c, int32_t* sizes_host, int32_t* members_host);
/* For every row r < n_rows of the batch set on engine h (a forward is run if none has been): the row's cluster
 * c = argmax_j (u_r . Wc)[j] (what sbr_cluster_select returns), the scores h_last[r] . W_out^T[i] + b_out[i] of i in members(c) only,
 * and their ordered top-k.  Exclusion (exclude_input, excl_ids / excl_off), validation, k, the order of the result, its -1 / -inf
 * places (also k above the cluster's size, and an empty cluster) and the scratch are those of sbr_rank above; an excluded id outside the
 * row's cluster is ignored.  On the default projection a score is the very float sbr_rank ranks for (r, i), so the result equals
 * sbr_rank's filtered to members(c) -- bit for bit.
 *   ids_host      [n_rows][k];  scores_host  NULL or [n_rows][k]
 *   cluster_host  NULL or [n_rows]: the selected cluster;  size_host  NULL or [n_rows]: len(members(c)) before exclusion (the reference's
 *                 number of scored items, test.py:73-76)
 * c and h must agree in n_items, in the width and split of the user representation and in the stream (SBR_EINVAL); no batch set:
 * SBR_ESTATE.  Parameters, gradients and optimizer state stay untouched beyond bringing lazily stepped output rows up to date.
 * Two forms: 1 scores only the members (default); 2 runs the full projection and picks the members' scores out of it -- taken with
 * SBR_CLUSTER_RANK=0 in the environment at the engine's creation, with SBR_FLAG_BF16_PROJECTION and with SBR_FLAG_SIMPLE_GEMM.
 * sbr_query "cluster_rank_form" tells which the last call took (0: none yet), "rank_select" / "rank_sort" its regimes. */
int sbr_cluster_rank(sbr_cluster* c, sbr_handle* h, int k, int exclude_input, const int32_t* excl_ids, const int64_t* excl_off,
                     int32_t* ids_host, float* scores_host, int32_t* cluster_host, int32_t* size_host);

/* predict_function(X, mask) (rnn_base.py:188-194) on the current batch: scores (rows,N);
 * softmax probabilities for CCE (DenseLayer softmax, rnn_one_hot.py:65), raw activations
 * for the sampled heads (sparse_lstm.py:37-40).  probs != 0 forces softmax (test function of
 * the sampled heads, rnn_sampling.py:144).  out_host (rows*N floats) may be NULL. */
int sbr_predict_scores(sbr_handle* h, int probs, float* out_host);
/* test_function(theano_inputs, k) (rnn_base.py:196-211): ordered top-k ids per row of
 * softmax * (1 - exclude) where exclude = the row's own input items when exclude_seen
 * (interactions_are_unique, rnn_base.py:200-201).  Ties break to the lowest id.  A row with fewer than k rankable items
 * (more than N - k items excluded, or NaN scores) gets -1 in the places it cannot fill.
 *   k             1 <= k <= min(64, N)
 *   exclude_seen  0: nothing; 1: the items of the row's input window are never ranked (top_k_recommendations, rnn_base.py:154-155);
 *                 2: the compiled function's scores * (1 - exclude) (:201-202) -- 1's ranking for every loss but RNNMargin's, whose
 *                 raw outputs it ranks with the window items at 0.0 and still rankable
 * No batch set: SBR_ESTATE.  This is an entry to sbr_rank's pipeline (exclusion, radix select, sort) with the contract above: it
 * takes its select / sort working set from the handle's ranking scratch (see sbr_rank; SBR_ENOMEM when that cannot grow), an input
 * id outside [0, N) is skipped, the scores it ranks are left as the exclusion left them, and sbr_query "rank_select" / "rank_sort"
 * tell what it ran. */
int sbr_topk(sbr_handle* h, int k, int exclude_seen, int32_t* ids_host);
/* The same ranking, by the same kernels, without sbr_topk's limits (ABI 11): any depth 1 <= k <= N, and per-row exclusion lists -- the batched form of
 * top_k_recommendations(sequence, k, exclude=...) (rnn_base.py:140-165), for users whose history is longer than max_length (all of
 * it is excluded, only its end is fed) and for metrics deeper than 64.  The scores ranked are the ones sbr_topk ranks (the exact-f32
 * projection plus bias, no softmax: monotone), so the two calls agree id for id.
 *   exclude_input != 0   the items of each row's input window are never ranked (sbr_topk's exclude_seen = 1)
 *   excl_ids / excl_off  HOST arrays, a CSR over the batch's rows: excl_off has n_rows + 1 non-decreasing entries, row r's further
 *                        excluded ids are excl_ids[excl_off[r] .. excl_off[r + 1]) -- any length, duplicates and empty lists
 *                        allowed; both NULL: no lists.  An id outside [0, N), decreasing offsets, or exactly one of the two NULL
 *                        is SBR_EINVAL, found before anything is launched: the engine stays usable.
 *   ids_host             [n_rows][k], score descending, ties to the lowest id (-0.0 and +0.0 tie).  Finite scores and +inf are
 *                        ranked; NaN, -inf and excluded items never; the places a row cannot fill hold -1
 *   scores_host          NULL, or [n_rows][k]: the score of each ranked id (-inf in the unfilled places); softmax is NOT applied
 * No batch set: SBR_ESTATE.  The call needs scratch that grows with n_rows * k and the lists; it is the handle's own device
 * allocation (made on first use, grown on demand, freed by sbr_destroy), never part of the arena -- sbr_arena_bytes does not change.
 * A failed allocation is SBR_ENOMEM with the byte count in sbr_last_error().  Parameters, gradients and optimizer state are not
 * touched (beyond bringing lazily stepped rows up to date, as sbr_topk does).  sbr_query "rank_select" / "rank_sort" tell what the
 * last call ran: the select with the row in LDS (1) or streamed (2), the sort in LDS (1) or as a radix sort in scratch (2). */
int sbr_rank(sbr_handle* h, int k, int exclude_input, const int32_t* excl_ids, const int64_t* excl_off,
             int32_t* ids_host, float* scores_host);
/* sbr_rank restricted to a candidate list per row (added under ABI 11: two symbols, this one and sbr_sessions_rank_candidates below;
 * no struct change) -- "of these few hundred items, which k does the user want next?" behind a retrieval stage or a category page,
 * without scoring the whole catalogue.
 *   cand_ids / cand_off  HOST arrays, a CSR, both required.  shared == 0: cand_off has n_rows + 1 entries, row r's candidates are
 *                        cand_ids[cand_off[r] .. cand_off[r + 1]);  shared != 0: cand_off has 2 entries, one list for every row.
 *                        Every list is STRICTLY ASCENDING in id and inside [0, N); it may be empty and hold up to N ids (all lists of
 *                        a call together at most 2^31 - 1).
 *   ids_host             [n_rows][k], 1 <= k <= N: sbr_rank's ordered top-k of the row restricted to its list -- score descending,
 *                        ties to the lowest id; NaN, -inf and excluded ids are never ranked; the places a row cannot fill (k above
 *                        the list's length, an empty list) hold -1
 *   scores_host          NULL, or [n_rows][k]: raw scores, no softmax; -inf in the unfilled places
 *   exclude_input, excl_ids / excl_off   exactly sbr_rank's; an excluded id that is not in the row's list is ignored
 * On the default projection a score is the very float sbr_rank ranks for (row, item) -- the same instruction on the same operand
 * roles in the same k order, the same two adds -- so the call equals sbr_rank at k = N filtered to the row's list, id for id and bit
 * for bit.  Two forms: 1 scores only the candidates (per-row lists: cand_score_kernel; a shared list: sbr_cluster_rank's scoring
 * kernel with one cluster of all rows); 2 runs the full projection and picks the candidates' scores out of it -- taken with
 * SBR_CAND_RANK=0 in the environment at the engine's creation, with SBR_FLAG_BF16_PROJECTION and with SBR_FLAG_SIMPLE_GEMM.
 * sbr_query "cand_rank_form" tells which the last call took (0: none yet), "rank_select" / "rank_sort" its regimes.
 * No batch set: SBR_ESTATE.  SBR_EINVAL, found on the host before anything is launched, the offender named by row and position in
 * its list: cand_ids or cand_off NULL, negative or decreasing offsets, an id outside [0, N), a list that is not strictly ascending,
 * k or exclusion lists as sbr_rank rejects them; the engine stays usable and untouched.  A forward is run if the batch has none;
 * lazily stepped output rows are brought up to date (all of them, as sbr_rank does); parameters, gradients and optimizer state are
 * otherwise untouched.  Scratch: the handle's ranking scratch (see sbr_rank); sbr_arena_bytes does not change.  One wait, at the end. */
int sbr_rank_candidates(sbr_handle* h, int k, const int32_t* cand_ids, const int64_t* cand_off, int shared, int exclude_input,
                        const int32_t* excl_ids, const int64_t* excl_off, int32_t* ids_host, float* scores_host);

/* The dense GEMM of the hot path on caller-provided DEVICE buffers (parity tests of the kernels themselves):
 * C[m][n] = sum_k A[m*sam + k*sak] * B[k*sbk + n*sbn] (+ bias[n]); ws: split-K workspace (may be NULL).
 * exact_f32 = 1: v_mfma_f32_16x16x4_f32 kernel; 0: bf16x6 kernel where the shape allows it; 2: plain bf16 operands (the
 * SBR_FLAG_BF16_PROJECTION kernel); 3: the two-plane fp16 split, three MFMAs per product (operands within fp16's range: what the
 * step's logits / layer GEMMs take since ABI 8); 4 / 5: as 3 / 2 but kept on the 128-wide tile where the library would pick the
 * 256 x 128 one (gemm_x6w_kernel; the two give the same bits: tests/test_gpu_gemm.py). */
int sbr_debug_gemm(void* stream, const float* A, int64_t sam, int64_t sak, const float* B, int64_t sbk, int64_t sbn,
                   float* C, int64_t ldc, int32_t M, int32_t N, int32_t K, const float* bias, float* ws, size_t ws_floats,
                   int32_t exact_f32);

/* Named device buffers for parity tests: "h_last" (rows,Hp), "logits", "xt0", "hs0", "cs0" (LSTM: the cell states, laid out like hs0) ... */
int sbr_debug_buffer(sbr_handle* h, const char* name, void** dev_ptr, size_t* n_floats);
/* Copy n_floats from a device pointer to host (tests without torch). */
int sbr_copy_to_host(sbr_handle* h, const void* dev_ptr, float* host, size_t n_floats);
int sbr_synchronize(sbr_handle* h);

/* Per-phase device time of the train steps since sbr_enable_timing, in microseconds (hipEvents on the
 * handle's stream): gather, rec_fwd, output, rec_bwd, wgrad, scatter, update, total.
 * on = 0: off; 1: every phase (eight event records per step: each costs the stream a few microseconds, ~40 us per
 * C2 step); 2 + p: only phase p (two records; the others read 0) -- what bench.py uses inside its timed region. */
#define SBR_N_PHASES 8
int sbr_enable_timing(sbr_handle* h, int on);
/* Which kernels this handle's shapes select (tooling: bench.py names the kernels it prices):
 * "fused_gather" (layer-0 input rows gathered inside the forward kernel), "rows_per_workgroup",
 * "cluster" (multi-workgroup recurrent kernels for the top layer), "rec_kernel" (kernel family of the top layer:
 * 0 triage, 1 cluster, 2 counter-synchronised 128-unit, 3 counter-synchronised 32/64-unit, 4 barrier / general),
 * "arena_bytes", "side_stream" (hipStream_t), "sparse_blocks" (row-sparse parameter blocks of this configuration),
 * "adam_table" (entries of the a_t table of the lazy Adam catch-up); what the top layer's recurrent kernels put on the
 * matrix pipe, for roofline reports: "rec_products_fwd" / "rec_products_bwd" (low-precision MFMA terms per f32 product:
 * 6 = bf16x6, 3 = fp16x3, 0 = exact-f32 MFMA kernels), "rec_rows_fwd" / "_bwd" (live batch rows among the 16 columns of an
 * MFMA tile), "rec_workgroups_fwd" / "_bwd" (workgroups of the launch = CUs it can occupy); ABI 9: "head_fused" (column chunks of
 * the one-launch full-softmax head a full batch of a training step takes, 0 = the three launches: rnn_one_hot.py:65-71 forward +
 * backward); "head_sampled" (1: a full batch of a training step with a sampled
 * loss takes the one-launch head -- full 16-row blocks, 128 / 256 / 512 padded units, at most 320 cells = targets + samples --,
 * 0: the four launches; a key of the same ABI, no new symbol); what the LAST step launched, recorded where it is launched:
 * "scatter_form" (the scatter-add of layer 0's index-input gradient rows: -1 no step yet, 0 sorted segment reduce, 1 range form,
 * 2 segment-parallel form, 3 per-element atomics of SBR_FLAG_ATOMIC_SCATTER, 4 / 5 the overlapped tail's polling reduce / its
 * LDS-row kernel), "row_aware_update" (1: its optimizer pass over layer 0's W_in was the row-aware one), "tail_gate_first" (1: the side
 * stream of its overlapped tail was released by the gate on the BPTT chain's progress words at its head, 0: by a main-stream record),
 * "step_join_gate" / "step_fork_gate" (1: the step's end joined its consumer streams through the gate on their completion words /
 * its start released the second side stream by the forward chain's start word; 0: by events on the main stream). */
int sbr_query(sbr_handle* h, const char* what, int64_t* value);
int sbr_phase_times(sbr_handle* h, float us[SBR_N_PHASES]);
/* Chain-only timing (ABI 8; tooling: bench.py prices the recurrent chain kernels of stacked layers apart from the dense GEMMs
 * between them).  on = 1: from now on every launch of a recurrent chain kernel -- the compiled scan of sparse_lstm.py:425 /
 * recurrent_layers.py:57-68 and its gradient, any layer, either direction -- is bracketed by a HIP-event pair (up to 256 launches);
 * on = 0: stop and report us[0] / us[1] = device time summed over the forward / backward chain launches since the start,
 * n[0] / n[1] = the number of launches (us, n may be NULL with on = 1).  A survey facility: the records delay the stream. */
int sbr_chain_times(sbr_handle* h, int on, float us[2], int n[2]);
/* The scatter-add of the embedding gradient ON ITS OWN (ABI 9; tooling: bench.py's `kernels.scatter_unfused`, north_star "achieved
 * HBM GB/s on the embedding gather/scatter"): the gradient of sparse_lstm.py:368's gather (AdvancedIncSubtensor), layer 0's
 * dW_in[X[b][t][f]][:] += dxt[t][b][:] over the current batch, as the step's stand-alone form for this shape runs it -- counting
 * sort of the ids once, then `reps` launches of the scatter-add on the engine's stream between two HIP events, nothing beside
 * them; *us = mean microseconds per launch, *entries = valid (t, b, f) positions, *rows = distinct ids (gradient rows written).
 * dxt holds whatever the last backward pass left; the gradient block is cleared again afterwards.  Index-input layer 0 only. */
int sbr_debug_scatter(sbr_handle* h, int reps, float* us, int64_t* entries, int64_t* rows);
/* A FOREIGN kernel that holds part of the chip (ABI 10; test hook): `workgroups` workgroups of 256 threads, each claiming `lds_kb`
 * KiB of LDS, spin for `milliseconds` on a stream of the library's own (not the engine's) -- asynchronous, returns at once.  What the
 * tests use to show that a cluster chain whose workgroups cannot all be resident (rnn_base.py has no such notion: one process, one
 * Theano function) ends in the fault code of sbr_read_cost / sbr_train_step -- never in a wrong gradient -- and that the one-launch
 * head recomputes what it cannot wait for.  sbr_synchronize(h) does NOT wait for it; sbr_debug_occupy(h, 0, 0, 0) does. */
int sbr_debug_occupy(sbr_handle* h, int workgroups, int lds_kb, int milliseconds);

/* ------------------------------------------------------------------------------------------------
 * Native batch builder: replaces SequenceGenerator + _gen_mini_batch + _prepare_input
 * (data_handling.py:126-174, rnn_base.py:373-420, rnn_one_hot.py:83-106, rnn_sampling.py:159-194) for
 * the default training options (one item index per step, next-item target, no sequence noise).
 * The training sequences live on the device in CSR form; a pass over the users is PLANNED on the host
 * exactly as the reference fills its batches (users in file or shuffled order; user u contributes
 * k = min(B - j, len(u) - 2) rows, a user that overflows the batch is truncated, rnn_base.py:400-415),
 * and each batch is then BUILT by two kernels: k distinct sorted split points l in [2, len) per user
 * (uniform without replacement = random.sample, :402), then per row the window items[max(0,l-T):l], its
 * length, the target items[l], pop[target]**db and (sampled heads) S negatives, uniform or by inverse CDF
 * of popularity**sampling_bias.  Same distribution as the reference, not the same random stream. */
typedef struct sbr_dataset sbr_dataset;

/* items: concatenated item ids of all training sequences; offsets: n_users+1 prefix offsets (host arrays). */
int sbr_dataset_create(const int32_t* items, const int64_t* offsets, int64_t n_users, int32_t n_items, void* stream,
                       sbr_dataset** out);
int sbr_dataset_destroy(sbr_dataset* d);
/* pop_db[n_items] = item_popularity ** diversity_bias (rnn_one_hot.py:103; NULL: all 1);
 * sample_cdf[n_items] = cumsum(item_popularity ** sampling_bias) (rnn_sampling.py:159-163; NULL: uniform). */
int sbr_dataset_set_tables(sbr_dataset* d, const float* pop_db, const double* sample_cdf);
/* Options that shape a batch beyond the defaults.  ratings[nnz] (parallel to `items`, NULL = none): with --rf a step feeds the
 * item index and n_items + the rating's one-hot index round(rating * 2) - 1 (rnn_base.py:590-642; model built with n_feat = 2,
 * input_size = n_items + 10).  shuffle_targets != 0: --shuffle_targets -- a row's targets are a uniform random subset of the
 * whole remaining sequence instead of its first items (target_selection.py:45-46).  The number of targets per row is the
 * model's (n_targets of the multi-target losses, 1 otherwise). */
int sbr_dataset_set_options(sbr_dataset* d, const float* ratings, int shuffle_targets);
/* Sequence noise for the pass planned NEXT (SequenceNoise.__call__, sequence_noise.py:52-94; call before sbr_dataset_plan_pass,
 * once per pass): per user, in the reference's order -- dropout of items (a user left with fewer than two items yields no rows
 * this pass), swaps of neighbours with probability n_swap (an item swaps at most once), swaps with the item int(N(0, 1) *
 * shuf_std) places away with probability n_shuf, rating +- 0.5 clamped to [1, 5] with probability n_ratings (only with ratings
 * attached).  The batches of the pass read the noised copy; rows carried over from the previous pass are re-drawn from it.
 * All probabilities 0: the pass reads the sequences as they are.  A law, not the reference's random stream. */
int sbr_dataset_noise_pass(sbr_dataset* d, float dropout, float swap, float shuf, float shuf_std, float ratings_perturb, uint64_t seed);
/* --target_bias (SelectTargets, target_selection.py:36-53): keep_prob[n_items] = (min(pop) / pop) ** bias; a candidate target
 * survives with that probability, a row none of whose remaining items survives is skipped and does not count towards its batch
 * (rnn_base.py:404-409).  Which rows a pass has is then a draw, so with a table set the rows of a pass -- user, split point,
 * target positions -- are planned on the host at sbr_dataset_plan_pass (sbr_plan_rows_host below: the reference's procedure
 * with splitmix64 draws seeded from `seed` and the pass number) and uploaded; sbr_build_batch only packs them.  n_targets must
 * be the model's.  With sequence noise on, the rows a pass carries over are dropped (they index the previous pass's copy).
 * keep_prob == NULL switches back to device-drawn rows. */
int sbr_dataset_set_target_bias(sbr_dataset* d, const float* keep_prob, int32_t n_targets, uint64_t seed);
/* The host row planner (no device needed; used by the CPU tests).  items / offsets: the CSR of sbr_dataset_create; lengths:
 * NULL or the current length of every user's sequence (<= its CSR extent); order: NULL or the user order of the pass;
 * pend_*: rows carried in (n_pend < batch_size of them) and out; row_*: the rows of the complete batches, batch-major,
 * row_tgt[n_rows][n_targets] = positions inside the remaining sequence (items[offsets[u] + split + pos]), -1 behind the last. */
int sbr_plan_rows_host(const int32_t* items, const int64_t* offsets, const int64_t* lengths, const int32_t* order, int64_t n_users,
                       int32_t batch_size, int32_t n_targets, int32_t shuffle, const float* keep_prob, uint64_t seed,
                       int32_t* pend_user, int32_t* pend_split, int32_t* pend_tgt, int32_t* n_pend, int64_t cap_rows,
                       int32_t* row_user, int32_t* row_split, int32_t* row_tgt, int64_t* n_rows, int64_t* n_batches);
/* (tests / tooling) the sequences the next planned pass reads: items[nnz] and rating_index[nnz] (may be NULL) in the CSR layout
 * of sbr_dataset_create -- user u's items[offsets[u] .. offsets[u] + lengths[u]) -- and lengths[n_users]; the noised copy behind
 * sbr_dataset_noise_pass, the sequences as uploaded otherwise. */
int sbr_dataset_current_sequences(sbr_dataset* d, int32_t* items, int32_t* rating_index, int32_t* lengths);
/* Plans one pass over the users in `order` (n_users ids, NULL = file order) for batches of batch_size rows.
 * A trailing partial batch is carried into the next planned pass, as the reference's endless generator does.
 * n_batches: complete batches now available (indices 0..n_batches-1 for sbr_build_batch). */
int sbr_dataset_plan_pass(sbr_dataset* d, const int32_t* order, int32_t batch_size, int64_t* n_batches);
/* The plan as host arrays, for tests and tooling: segment s = (user, k rows, first row, batch). */
int sbr_dataset_plan_segments(sbr_dataset* d, int64_t* n_segments, const int32_t** seg_user, const int32_t** seg_k,
                              const int32_t** seg_row0, const int32_t** seg_batch);
/* Host-only planner behind sbr_dataset_plan_pass (no device needed; used by the CPU tests).  lengths[n_users];
 * pend_*: the carried partial batch (in/out, capacity batch_size); seg_* capacity n_users + *n_pend. */
int sbr_plan_pass_host(const int64_t* lengths, const int32_t* order, int64_t n_users, int32_t batch_size,
                       int32_t* pend_user, int32_t* pend_k, int32_t* n_pend, int32_t* seg_user, int32_t* seg_k,
                       int32_t* seg_row0, int32_t* seg_batch, int64_t* n_segments, int64_t* n_batches);
/* Builds planned batch `batch` into the engine's own batch buffers (rows [row_offset, row_offset+local_batch)
 * of the global batch for X / lengths / pop; targets: local rows for CCE, all rows for the sampled heads) and
 * makes it the current batch, as sbr_set_batch does.  Entirely on the handle's stream; no host sync. */
int sbr_build_batch(sbr_handle* h, sbr_dataset* d, int64_t batch, uint64_t seed);

/* ------------------------------------------------------------------------------------------------
 * Evaluation of whole users on the device (added under ABI 11: one symbol, no struct change) -- the per-user loops of test.py:43-77
 * and of the validation inside train() (rnn_base.py:358-371; evaluation.py:16-216) for a list of users in ONE call.  User
 * u = users[j] is sequence u of d as uploaded (never the noised copy; no planned pass is touched): L = its length, half = L / 2, the
 * viewed half is items[0 .. half), the goal items[half .. L) (test.py:81-83, _gen_mini_batch(test=True)); the row fed is the last
 * min(T, half) viewed items, left-aligned and padded with index 0 (+ n_items + rating index with n_feat == 2, ratings attached by
 * sbr_dataset_set_options).  local_batch users at a time are packed into the engine's batch buffers (the handle is left as
 * sbr_set_batch leaves it), scored (the very floats sbr_rank ranks), excluded straight from the dataset's device CSR, ranked by
 * sbr_rank's kernels (sbr_query "rank_select" / "rank_sort" report them) and compared with the goal; everything is enqueued on the
 * engine's stream without a host wait in between, and the call waits for the device once, at its end.
 * users may repeat, in any order.  SBR_EINVAL, found before anything is launched (the engine stays usable): a user outside
 * [0, n_users) or with L < 2, n < 1, k outside [1, N], an unknown mode, n_feat == 2 without ratings attached, items or stream of h and
 * d that differ.  Parameters, gradients and optimizer state are touched only by bringing lazily stepped rows up to date, as sbr_rank
 * does.  Scratch: the handle's ranking scratch (see sbr_rank), grown once per call. */
#define SBR_EVAL_EXCL_NONE 0         /* --repeated_interactions */
#define SBR_EVAL_EXCL_VIEWED 1       /* the whole viewed half is never ranked, also the part that no longer fits the window
                                        (top_k_recommendations, rnn_base.py:132-159; test.py:43-77) */
#define SBR_EVAL_EXCL_WINDOW 2       /* only the items fed are never ranked (the compiled test function, rnn_base.py:196-209: validation) */
#define SBR_EVAL_EXCL_WINDOW_ZERO 3  /* the items fed score 0.0 and stay rankable (the same function on RNNMargin's raw outputs: sbr_topk's exclude_seen = 2) */
int sbr_evaluate(sbr_handle* h, sbr_dataset* d, const int32_t* users, int64_t n, int k, int exclude_mode,
                 int32_t* ids_host,        /* NULL, or [n][k]: exactly sbr_rank's ids (-1 in unfilled places) */
                 int32_t* n_pred_host,     /* [n] places filled (ids >= 0) */
                 int32_t* hits_host,       /* [n] |set(goal) & set(top-k)| */
                 int32_t* first_hit_host,  /* [n] 1 when goal[0] is among the top-k (sps) */
                 uint32_t* hitmask_host,   /* NULL, or [n][(k + 31) / 32]: bit p of a row = the id at place p is a goal item */
                 int32_t* item_hits_host); /* NULL, or [N]: over all n users, how often item i was a correct prediction */

/* ------------------------------------------------------------------------------------------------
 * The rank of every goal item on the device (added under ABI 11: one symbol, no struct change) -- what test.py:42-77 with
 * get_full_recommendation_list and evaluation.py:198-206 (get_rank_comparison) obtain per user from a ranking to depth N, and what
 * the metrics at ANY depth follow from.  Users are split, fed, chunked (local_batch per chunk) and excluded exactly as by
 * sbr_evaluate, in all four SBR_EVAL_EXCL_* modes (WINDOW_ZERO leaves the items fed at 0.0 and rankable); users may repeat; the
 * handle is left as sbr_set_batch leaves it.  For user users[j] and goal place p (sequence order, p < L - L / 2), with g the item there:
 *   ranks[goal_off[j] + p]   the place of g in sbr_rank's result at k = N for that row: the number of rankable items i with a better
 *                            score, or an equal score and i < g; -1 when g itself is never ranked (excluded, NaN, -inf, outside
 *                            the catalogue).  A goal that repeats an item holds the same rank at each of its places.
 *   n_rankable[j]            the rankable items of the row = sbr_evaluate's n_pred at k = N.
 * A rank is a count (ev_goal_rank_kernel, sbr_eval.hip): one pass over the score row per 1024 goal items (sbr_query "goal_rank_tile"),
 * no select, no sort, no k; integer arithmetic only.  sbr_query "goal_rank_form": 1 the row's keys stayed in LDS, 2 every pass streamed
 * the row (N > 32768), 0 no call yet.  Every chunk is enqueued on the engine's stream without a host wait in between; the call waits
 * once, at its end.  goal_off is computed on the host from the lengths and written before anything is launched.
 * SBR_EINVAL, found before anything is launched (the engine stays usable): everything sbr_evaluate rejects (k does not exist here), an
 * unknown mode, a NULL output, cap < goal_off[n] (sbr_last_error names the count needed).  Parameters, gradients and optimizer state
 * are the same bits after the call as before it: lazily stepped rows are brought up to date for the call as by sbr_evaluate, and
 * -- since where the replay of their missed steps is split changes float32 roundings -- put back behind the last chunk, so that
 * training goes on exactly as if the call had not been made (also when a chunk fails to launch; not when one of these copies itself
 * fails, SBR_EHIP: the rows are then left up to date, which is valid state).  That copy is (1 + optimizer state arrays) x parameters
 * floats of ranking scratch and twice that in device traffic per call, only on an engine that steps rows lazily and has trained
 * (LSTM-256 on 100 000 items with Adam: 1.5 GB, one millisecond per call -- profiles/eval_ranks_bench.json).  Scratch: the handle's ranking scratch (users, n + 1 offsets,
 * goal_off[n] ranks, n counts; with lazily stepped rows and steps applied, the copy of parameters and optimizer state). */
int sbr_evaluate_ranks(sbr_handle* h, sbr_dataset* d, const int32_t* users, int64_t n, int exclude_mode,
                       int64_t* goal_off_host,     /* [n + 1]: user j's goal places are [goal_off[j], goal_off[j + 1]); goal_off[0] = 0 */
                       int32_t* ranks_host,        /* [cap] */
                       int64_t cap,                /* must be >= goal_off[n] = sum over users of L - L / 2 */
                       int32_t* n_rankable_host);  /* [n] */

/* ------------------------------------------------------------------------------------------------
 * The rank of the NEXT item at every position of a sequence (added under ABI 11: one symbol and one constant, no struct change) --
 * sbr_evaluate_ranks' sibling.  Where every other evaluation call asks one question per user (split in the middle, rank once), this
 * one reads every state ONE forward pass leaves.  User users[j] has items x_0 .. x_{L-1}; T = max_length, m = min_history >= 1:
 *   fed        the first F = min(L - 1, T) items, from the START of the sequence (not the window of the viewed half);
 *   positions  p = m .. F: the state is slot p of the top layer (the state after p items), the goal is x_p;
 *   count      n_pos(j) = max(0, F - m + 1); positions beyond T are not evaluated.
 * User j's results are [pos_off[j], pos_off[j + 1]), in order of p:
 *   ranks[pos_off[j] + p - m]       the number of rankable items i with a better score than x_p, or an equal score and i < x_p, among
 *                                   the scores sbr_rank would rank for a row fed x_0 .. x_{p-1} (the same projection launches, the
 *                                   same order: key descending, ties to the lowest id); -1 when x_p itself is not rankable (NaN,
 *                                   -inf, excluded, outside the catalogue);
 *   n_rankable[pos_off[j] + p - m]  the rankable items at that position.
 * exclude_mode: SBR_EVAL_EXCL_NONE, or SBR_EVAL_EXCL_PREFIX: the distinct ids among x_0 .. x_{p-1} are not rankable at position p --
 * what SBR_EVAL_EXCL_VIEWED means for a user whose viewed half is that prefix.  The two agree, value for value, with
 * sbr_evaluate_ranks (NONE / VIEWED) on an explicit user x_0 .. x_{p-1}, x_p padded to length 2p or 2p + 1 (tests/test_gpu_eval_positions.py).
 * Per chunk of local_batch users: pack, one forward pass, first-occurrence flags of the rows, then per group of consecutive positions
 * one projection of their slots (sbr_query "next_rank_slots": up to 8 per GEMM launch where their scores fit 64 MB of scratch; 1 under
 * SBR_FLAG_BF16_PROJECTION, whose kernel chooses its tile by the row count) and one counting launch (ev_next_rank_kernel,
 * sbr_eval.hip: one streamed pass over the N scores per row and position, integer counts, nothing written to the scores; sbr_query
 * "next_rank_form": 1 16-byte loads, 2 4-byte loads -- N no multiple of 4 --, 0 no call yet).  Everything on the engine's stream, no host wait between; the call waits once, at its end.  users may repeat;
 * the handle is left as sbr_set_batch leaves it.  pos_off follows from the lengths alone: computed on the host and written before
 * anything is launched.
 * SBR_EINVAL, found before anything is launched (nothing but pos_off -- and that only once cap is known to suffice -- is written, the
 * engine stays usable): everything sbr_evaluate rejects (k does not exist here), a mode other than the two above, min_history < 1, a
 * bidirectional engine (a backwards layer's state at p has seen what lies behind p), a NULL output, cap < pos_off[n]
 * (sbr_last_error names the count needed).  Parameters, gradients and optimizer state are the same bits after the call as before
 * it, by the keep-and-restore sbr_evaluate_ranks describes.  Scratch: the handle's ranking scratch (users, n + 1 offsets, twice
 * pos_off[n] words, local_batch x T flags, the scores of a group of slots; the copy of parameters and optimizer state as for sbr_evaluate_ranks). */
#define SBR_EVAL_EXCL_PREFIX 4       /* sbr_evaluate_positions only: at position p the distinct items of x_0 .. x_{p-1} are never ranked */
int sbr_evaluate_positions(sbr_handle* h, sbr_dataset* d, const int32_t* users, int64_t n, int min_history, int exclude_mode,
                           int64_t* pos_off_host,      /* [n + 1]: user j's positions are [pos_off[j], pos_off[j + 1]); pos_off[0] = 0 */
                           int32_t* ranks_host,        /* [cap] */
                           int32_t* n_rankable_host,   /* [cap] */
                           int64_t cap);               /* must be >= pos_off[n] = sum over users of max(0, min(L - 1, T) - min_history + 1) */

/* ------------------------------------------------------------------------------------------------
 * The log-probability of held-out items on the device (added under ABI 11: three symbols, no struct change) -- the validation loss:
 * where every call above answers a ranking question, these two give the full-softmax log-likelihood of the same goal items from the
 * same score rows.  For one score row of N floats, with "rankable" the counting kernels' rule (not NaN, not -inf,
 * not excluded), m the largest rankable score and S the sum over the rankable items of exp(s_i - m):
 *   log_z    = m + log(S)                   -inf for a row without a rankable item
 *   logp(g)  = (s_g - m) - log(S)           -inf where g is not rankable (excluded, NaN, -inf, an id outside [0, N))
 * A +inf score is rankable and makes m = +inf: log_z and every logp of that row are NaN.  s_g - m beyond the float range is -inf.
 * The scores are the floats sbr_rank ranks (raw outputs, biased; whatever the head was trained with), so the number compares models
 * as probability models.  Exclusion is a WRITE of -inf into the row before the reduction, never a subtraction from a finished sum.
 * The float additions run in an order fixed by N alone (row_log_z, sbr_eval.hip: 256 threads whatever the launch, each adding its
 * groups of four items in ascending order, then a fixed tree of depth 8; no atomics): a row's log_z and logp are the same bits
 * whichever users, chunks, slots or groups share the call, and the same in all three calls.  |log_z - exact| <=
 * (4 * ceil(ceil(N / 4) / 256) + 8 + 8) * 2^-24 for |log_z| < 16.  sbr_query "logprob_form": 1 the rows were read in 16-byte loads,
 * 2 in 4-byte loads (N no multiple of 4), 0 no call yet -- the bits do not depend on it.
 *
 * sbr_evaluate_logprob is sbr_evaluate_ranks' call: the same split, window, chunks, offsets (goal_off), repeated users, one wait at
 * the end, keep-and-restore of lazily stepped rows, and errors; exclude_mode SBR_EVAL_EXCL_NONE, _VIEWED or _WINDOW (_WINDOW_ZERO is
 * SBR_EINVAL: an item scored 0.0 has not left the softmax).  logp[goal_off[j] + p] belongs to goal place p of users[j], log_z[j] to
 * its row.  ranks / n_rankable, where given, are exactly sbr_evaluate_ranks' (its kernel runs on the same rows in the same call).
 * sbr_evaluate_positions_logprob is sbr_evaluate_positions' call in the same way (SBR_EVAL_EXCL_NONE or _PREFIX; bidirectional
 * engines are refused): logp, log_z, ranks and n_rankable at pos_off[j] + p - min_history.  Under _PREFIX the ids of x_0 .. x_{p-1}
 * are written -inf into the position's own score row (behind the integer counts, which read the row as projected).  On an explicit
 * user x_0 .. x_{p-1}, x_p padded to length 2p or 2p + 1 sbr_evaluate_logprob gives the same bits (NONE / VIEWED).
 * Both: SBR_ESTATE inside an open training step or with a lagged cost pending.
 * sbr_debug_row_logprob is the test hook of the reduction: the same device function on rows [rows][ld] of DEVICE scores (only read),
 * goal_ids_dev [rows][goals_per_row], results into logp_dev [rows][goals_per_row] and log_z_dev [rows] (NULL: not written); on the
 * engine's stream, waits for the device. */
int sbr_evaluate_logprob(sbr_handle* h, sbr_dataset* d, const int32_t* users, int64_t n, int exclude_mode,
                         int64_t* goal_off_host,     /* [n + 1], as sbr_evaluate_ranks writes it */
                         float* logp_host,           /* [cap] */
                         int64_t cap,                /* must be >= goal_off[n] */
                         float* log_z_host,          /* NULL, or [n] */
                         int32_t* ranks_host,        /* NULL, or [cap]: exactly sbr_evaluate_ranks' */
                         int32_t* n_rankable_host);  /* NULL, or [n] */
int sbr_evaluate_positions_logprob(sbr_handle* h, sbr_dataset* d, const int32_t* users, int64_t n, int min_history, int exclude_mode,
                                   int64_t* pos_off_host,      /* [n + 1], as sbr_evaluate_positions writes it */
                                   float* logp_host,           /* [cap] */
                                   float* log_z_host,          /* NULL, or [cap] */
                                   int32_t* ranks_host,        /* NULL, or [cap]: exactly sbr_evaluate_positions' */
                                   int32_t* n_rankable_host,   /* NULL, or [cap] */
                                   int64_t cap);               /* must be >= pos_off[n] */
int sbr_debug_row_logprob(sbr_handle* h, const float* scores_dev, int64_t ld, int64_t rows, int32_t N, const int32_t* goal_ids_dev,
                          int32_t goals_per_row, float* logp_dev, float* log_z_dev);

/* ------------------------------------------------------------------------------------------------
 * The rank of every goal item among a candidate set of its user (added under ABI 11: two symbols and one constant, no struct change)
 * -- the protocol of the sequential-recommendation papers: each positive against S negatives the user never interacted with, HR@k /
 * NDCG@k / MRR from the ranks -- without scoring the whole catalogue.  Users are split, fed and chunked (local_batch per chunk)
 * exactly as by sbr_evaluate_ranks; users may repeat; the handle is left as sbr_set_batch leaves it.  The candidate set C_j of
 * users[j] comes from exactly one of two sources:
 *   explicit   cand_ids / cand_off: HOST arrays, a CSR with n + 1 offsets as sbr_rank_candidates takes it (shared == 0): every list
 *              strictly ascending in id, inside [0, N), possibly empty, up to N ids; n_negatives = 0, neg_cdf and negatives_host NULL;
 *   sampled    cand_ids = cand_off = NULL, 1 <= n_negatives <= min(N - 1, SBR_EVAL_MAX_NEGATIVES): drawn on the device by a rule the
 *              host restates (sbr_eval_negatives_host).  With s_u = mix64(seed ^ mix64(0xCA4D + u)), u the user's id in the dataset
 *              (not its place in the call) and mix64 the splitmix64 finaliser, attempt t = 0, 1, .. draws item
 *              r_t % N (neg_cdf NULL: uniform) or the first i with neg_cdf[i] > (r_t >> 11) * 2^-53 * neg_cdf[N - 1] (neg_cdf: HOST
 *              [N], non-decreasing with positive mass, as sbr_dataset_set_tables checks sample_cdf), r_t = mix64(s_u ^ mix64(0xA5A5 + t))
 *              -- the law of the batch builder's negatives.  An attempt is accepted when its item occurs nowhere in user u's uploaded
 *              sequence (viewed or goal) and was not accepted before; the draw ends at n_negatives accepted or after
 *              16 * n_negatives + 256 attempts, so a row may hold fewer (n_cand and negatives say so).  The list depends on
 *              (seed, u, n_negatives, neg_cdf) only: not on the chunk, the order or the repetition of users.
 * For goal place p (sequence order, p < L - L / 2), with g the item there:
 *   ranks[goal_off[j] + p]   the number of rankable i in C_j that stand before g in sbr_rank's order (key descending, ties to the lowest
 *                            id); -1 when g itself is not rankable (NaN, -inf, excluded by the mode, outside the catalogue).  g need
 *                            not be in C_j; a goal item competes with the list alone, not with the other goal items (unless the list
 *                            names them); a goal that repeats an item holds the same rank at each of its places.
 *   n_cand[j]                the rankable members of C_j.
 *   negatives[j][..]         NULL, or (sampled only) [n][n_negatives]: the accepted ids in draw order, -1 behind the last.
 * With C_j = all N items, ranks and n_cand are sbr_evaluate_ranks' ranks and n_rankable.
 * exclude_mode: SBR_EVAL_EXCL_NONE, _VIEWED or _WINDOW -- an excluded item is neither ranked as a goal nor counted as a candidate;
 * _WINDOW_ZERO is SBR_EINVAL (a 0.0 for the items fed exists in the whole-catalogue matrix only).
 * Per chunk: pack, forward, ev_cand_build_kernel ([the draw,] candidates and distinct goal ids merged ascending into a device CSR),
 * the scores of those ids by sbr_rank_candidates' two forms -- 1: cand_score_kernel, on the default projection the very floats sbr_rank
 * ranks; 2: the full projection, gathered (SBR_CAND_RANK=0, SBR_FLAG_BF16_PROJECTION, SBR_FLAG_SIMPLE_GEMM) --, ev_cand_place_kernel
 * (exclusion from the dataset's CSR, then integer counts; sbr_eval_cand.hip).  sbr_query "eval_cand_form": the form of the last call
 * (0: none yet); "eval_cand_lmax": the width of its last chunk's compact score matrix.  goal_off is computed on the host and written
 * before anything is launched; everything is enqueued on the engine's stream and the call waits once, at its end (explicit lists are
 * uploaded once, in front of the first chunk, as sbr_rank_candidates uploads them).
 * SBR_EINVAL, found on the host before anything is launched (nothing but goal_off -- and that only once cap is known to suffice -- is
 * written, the engine stays usable): everything sbr_evaluate_ranks rejects, both or neither candidate source, a bad CSR (the offender
 * named by user and position, as sbr_rank_candidates names it), n_negatives or neg_cdf out of bounds, neg_cdf or negatives_host
 * together with explicit lists, cap < goal_off[n].  SBR_ESTATE inside an open training step.  Parameters, gradients and optimizer
 * state are the same bits after the call as before it, by the keep-and-restore sbr_evaluate_ranks describes.  Scratch: the handle's
 * ranking scratch (the lists, per chunk the merged lists and local_batch x width scores; the copy of parameters as for sbr_evaluate_ranks). */
#define SBR_EVAL_MAX_NEGATIVES 4096
int sbr_evaluate_candidates(sbr_handle* h, sbr_dataset* d, const int32_t* users, int64_t n, int exclude_mode,
                            const int32_t* cand_ids, const int64_t* cand_off,   /* explicit, or both NULL */
                            int32_t n_negatives, uint64_t seed, const double* neg_cdf,   /* sampled, or 0 / ignored / NULL */
                            int64_t* goal_off_host,     /* [n + 1], as sbr_evaluate_ranks */
                            int32_t* ranks_host,        /* [cap] */
                            int64_t cap,                /* must be >= goal_off[n] */
                            int32_t* n_cand_host,       /* [n] */
                            int32_t* negatives_host);   /* NULL, or [n][n_negatives] (sampled only) */
/* The draw above for ONE user, restated on the host (pure host code: no device, no handle) -- the documented way to reproduce a
 * published candidate set.  seq [L]: the user's whole uploaded sequence; out [n_negatives]: the accepted ids in draw order, -1 behind
 * the last; *n_out: how many were accepted.  SBR_EINVAL: a NULL output, n_negatives or neg_cdf out of the bounds above. */
int sbr_eval_negatives_host(const int32_t* seq, int32_t L, int32_t user, int32_t n_items, int32_t n_negatives, uint64_t seed,
                            const double* neg_cdf, int32_t* out, int32_t* n_out);

/* ------------------------------------------------------------------------------------------------
 * Evaluation of whole users of a cluster model on the device (added under ABI 11: one symbol and one struct, nothing existing
 * changes) -- sbr_evaluate for `--clusters C`: RNNCluster._compute_validation_metrics (rnn_cluster.py:409-438, one compiled test
 * function call per user) and test.py:61-76 (one top_k_recommendations call per user).  Users are split, fed, chunked
 * (local_batch per chunk) and compared with the goal exactly as by sbr_evaluate; the handle is left as sbr_set_batch leaves it;
 * everything is enqueued on the engine's stream and the host waits once, at the end of the call.  A row's cluster is what
 * sbr_cluster_select returns for it.
 *   whole    when given: exactly what sbr_evaluate returns for the same users, k and exclude_mode -- from the same forward pass.  (On
 *            the PRODUCT road of a margin loss, SBR_EVAL_EXCL_WINDOW ranks the whole catalogue as SBR_EVAL_EXCL_WINDOW_ZERO, the
 *            compiled test function's arithmetic on raw outputs.)
 *   inside, SBR_CEVAL_LISTS    per chunk exactly sbr_cluster_rank's ids for the packed rows: only the members of the row's cluster
 *            are ranked, score descending, ties to the lowest id, -1 behind the rankable members (k may exceed a cluster's size; a
 *            cluster may be empty), n_pred < k then.  SBR_EVAL_EXCL_VIEWED: the whole viewed half is never ranked; _WINDOW: the
 *            items fed; _NONE: nothing; read from the dataset's device CSR, no list is built or uploaded.  Both forms of
 *            sbr_cluster_rank stay, chosen by the same switches; sbr_query "cluster_rank_form" reports the one taken.
 *   inside, SBR_CEVAL_PRODUCT  the N scores p * m of a row are ranked by sbr_rank's kernels, p the float sbr_predict_scores with
 *            probs = 1 writes for (row, item) -- the same device code computes it --, m the float sbr_cluster_hard holds at
 *            [item][cluster of the row], the product one f32 multiply.  SBR_EVAL_EXCL_WINDOW: the items fed score +0.0 and stay
 *            rankable; _NONE: every score as it is.  size_host must be NULL.
 * The hits of both rankings follow sbr_evaluate's rule.  SBR_EINVAL, found before anything is launched (engine and head stay usable):
 * everything sbr_evaluate rejects, everything sbr_cluster_rank rejects about c against h (items, width and split, stream), a mode
 * the road does not take (LISTS: _WINDOW_ZERO; PRODUCT: _VIEWED, _WINDOW_ZERO), inside == NULL, a NULL n_pred / hits / first_hit in
 * a given sbr_eval_out, size_host on the PRODUCT road.  Parameters, gradients and optimizer state of engine and head are touched
 * only by bringing lazily stepped output rows up to date and by building the member lists (LISTS) or the membership matrix and its
 * transposed copy (PRODUCT) for the current R.  Scratch: the handle's ranking scratch, sized once per call.
 * Host waits besides the one at the end, all BEFORE the first chunk is enqueued and none between chunks: the ranking scratch growing
 * (hipFree / hipMalloc), the first call for a dataset (its sorted goals are uploaded), and once per version of R the member lists
 * (LISTS: their sizes are read back) or, on the first PRODUCT call of a head, the hipMalloc of the transposed copy (N * C floats). */
typedef struct sbr_eval_out {          /* one ranking's results, as the host outputs of sbr_evaluate */
    int32_t* ids;        /* NULL or [n][k] */
    int32_t* n_pred;     /* [n] */
    int32_t* hits;       /* [n] */
    int32_t* first_hit;  /* [n] */
    uint32_t* hitmask;   /* NULL or [n][(k+31)/32] */
    int32_t* item_hits;  /* NULL or [N] */
} sbr_eval_out;
#define SBR_CEVAL_LISTS   0   /* test.py:61-76 / top_k_recommendations: rank inside members(c), the lists of sbr_cluster_lists */
#define SBR_CEVAL_PRODUCT 1   /* the compiled test function, rnn_cluster.py:327-352: rank softmax * f(100 R)[:, c] over the catalogue */
int sbr_cluster_evaluate(sbr_cluster* c, sbr_handle* h, sbr_dataset* d, const int32_t* users, int64_t n, int k,
                         int road, int exclude_mode,
                         const sbr_eval_out* whole,    /* NULL, or the whole-catalogue ranking of the same forward pass */
                         const sbr_eval_out* inside,   /* required: the cluster ranking */
                         int32_t* cluster_host,        /* [n] selected cluster */
                         int32_t* size_host,           /* NULL or [n]: len(members(c)) (LISTS road) */
                         int32_t* cluster_use_host);   /* NULL or [C]: users per selected cluster */

/* ------------------------------------------------------------------------------------------------
 * One training iteration of a cluster model on a device-built batch (added under ABI 11: two symbols, no struct change) -- what
 * RNNCluster.train_function does per batch (rnn_cluster.py:277-287, :354-407), without a host copy and without a wait:
 *   1. sbr_train_step_lagged(h, prev_cost, have_prev): the network steps on the engine's current batch; its cost comes back one call
 *      late through the same slots, sbr_lagged_flush serves it;
 *   2. sbr_cluster_forward_backward on the user representation of that step's forward, with the B targets of that batch (the
 *      engine's own device buffer) and
 *        n_cluster_samples == 0   the S negatives of that batch (`cluster_samples = samples`, rnn_cluster.py:384, :392),
 *        n_cluster_samples  > 0   that many ids drawn on the device by d's law -- uniform, or the inverse of d's CDF table
 *                                 (sbr_dataset_set_tables) -- from `seed`: a draw of its own, independent of the batch's negatives.
 *      One launch writes targets ++ cluster samples into the head's id list, drawing where asked;
 *   3. sbr_cluster_apply_update(c).
 * Everything is enqueued on the engine's stream behind the step; nothing is synchronised.  SBR_ESTATE: no batch set.  SBR_EINVAL,
 * found before anything is launched (parameters, gradients and state of engine and head stay untouched): c against h as for
 * sbr_cluster_rank (items, width and split, stream), d against h (items, stream), a head whose batch_size is not the engine's, an
 * engine whose loss is not a sampled one, local_batch != batch_size or a batch of fewer rows (the head is single-rank and reads
 * every row), n_cluster_samples outside [0, max_samples], n_cluster_samples == 0 with S > max_samples. */
int sbr_cluster_train_step_lagged(sbr_cluster* c, sbr_handle* h, sbr_dataset* d, int n_cluster_samples, uint64_t seed,
                                  float* prev_cost, int* have_prev);
/* The id list of the head's last forward/backward (tests and tooling): targets ++ cluster samples, J = B + samples entries.
 * ids_host [n], n == J.  Synchronises the stream.  SBR_ESTATE: no forward/backward yet. */
int sbr_cluster_last_ids(sbr_cluster* c, int32_t* ids_host, int n);

/* ------------------------------------------------------------------------------------------------
 * Training state (added under ABI 11: nine symbols, no struct change) -- what a run needs beside the reference's checkpoint
 * (rnn_base.py:470-515 pickles the parameter arrays only) to go on, in a new process, bit for bit as if it had never stopped.
 * Three objects, each with   *_state_bytes(obj, &bytes)   the exact size of its blob now,
 *                            *_state_save(obj, blob_host, cap, &written)   cap >= bytes, written == bytes,
 *                            *_state_load(obj, blob_host, bytes).
 * A blob is host memory, opaque, little endian, and starts with a magic, a format version, its kind and its own size.
 * save changes nothing and launches nothing: it waits for the object's streams and copies device memory to the host -- lazily
 *   stepped rows (see "Row-sparse blocks") are NOT brought up to date, they are saved as they stand with their `last` words, so a
 *   run with saves in it computes what the run without them computes.
 * load checks the whole blob before it writes anything -- size, magic, version, kind, and what fixes the layout -- and returns
 *   SBR_EINVAL with the first mismatch in sbr_last_error(), the object untouched.  It never flushes either.
 *
 * sbr_state_*          the engine: parameter section as it lies in the arena (padding included), every optimizer state array, the
 *                      step count (Adam's t), every row-sparse block's `last` words.  Layout fingerprint: parameter floats, offset of
 *                      the output layer, number of state arrays, updater, kind / rows / row width of every sparse block, a hash of
 *                      the logical shapes of the parameter list (20 and 30 units pad to one layout: still two models) -- nothing of
 *                      local_batch or row_offset, data-parallel replicas hold the same state and read the same blob.
 *                      save: SBR_ESTATE while a training step is open (between sbr_zero_grads and sbr_apply_update) or a lagged
 *                      cost is pending (collect it with sbr_lagged_flush first).  load (SBR_ESTATE inside an open step) leaves a
 *                      fresh step boundary: gradient section zero, no current batch, no forward, no lagged report -- where a fresh
 *                      engine with these values stands.  save behind load returns the same bytes.
 * sbr_cluster_state_*  the cluster head: R, Wc, both optimizer state arrays of each, its step count, the noise counter, the scale as
 *                      sbr_cluster_set_scale left it, and the seed of its config.  load drops the hard clusters and the member lists,
 *                      as sbr_cluster_set_params does.  Fingerprint: items, clusters, features, updater.
 * sbr_dataset_state_*  what makes the next sbr_dataset_plan_pass reproduce its plan: the pass counter of the host row planner, the
 *                      rows (or users) the last planned pass carried over, the batch size they were planned for.  Host memory only.
 *                      NOT the sequences, tables and options: the caller sets those up from its files as on a fresh start (the target
 *                      bias included: the blob must agree with it), then loads.  Fingerprint: users, interactions, items; every
 *                      carried row must index the uploaded sequences.  The plan in force is left alone: plan the next pass. */
int sbr_state_bytes(sbr_handle* h, size_t* bytes);
int sbr_state_save(sbr_handle* h, void* blob_host, size_t cap, size_t* written);
int sbr_state_load(sbr_handle* h, const void* blob_host, size_t bytes);
int sbr_cluster_state_bytes(sbr_cluster* c, size_t* bytes);
int sbr_cluster_state_save(sbr_cluster* c, void* blob_host, size_t cap, size_t* written);
int sbr_cluster_state_load(sbr_cluster* c, const void* blob_host, size_t bytes);
int sbr_dataset_state_bytes(sbr_dataset* d, size_t* bytes);
int sbr_dataset_state_save(sbr_dataset* d, void* blob_host, size_t cap, size_t* written);
int sbr_dataset_state_load(sbr_dataset* d, const void* blob_host, size_t bytes);

/* ------------------------------------------------------------------------------------------------
 * Stateful sessions (added under ABI 11: symbols and three constants, no struct change) -- serving at the model's natural
 * cost.  Every ranking call above feeds a whole window of up to max_length items per row (rnn_base.py:140-165 does so per request); a
 * session pool KEEPS the recurrent state of `capacity` users, so that a user's next event costs one recurrent step and one projection.
 * A second object beside the engine, like the cluster head: its memory is its own device allocation (never part of the arena --
 * sbr_arena_bytes does not change): per layer two planes [capacity][Hp] of hidden states (and of cell states for LSTM; padded
 * units are kept as the chains keep them), per slot an event count and a ring of the ids of the last `history` events.
 *
 * A slot's state after p events is "the state after p items fed from the START of the sequence", the definition of
 * sbr_evaluate_positions (UserPrefix, not the window of UserSplit): there is no mask (every advance is an event) and NO WINDOW -- a
 * session carries its state over any number of events, which equals the windowed model of the other calls only while the events fit
 * max_length.
 *
 * Everything runs on the engine's stream.  reset / advance / replay / adopt enqueue and return without waiting for the device; rank and replay_ranks wait
 * once, at their end, like sbr_rank; read and write wait.  A call that reads parameters brings lazily stepped rows up to date first
 * (see "Row-sparse blocks": advance and replay the index-input block, rank and adopt the output rows, replay_ranks both), which moves float32 roundings of a
 * training run as sbr_rank does and is otherwise invisible to it; sessions keep states, not weights: after a training step they go on
 * under the new weights.  Inside an open training step (between sbr_zero_grads and sbr_apply_update) or with a lagged cost pending,
 * every call but read returns SBR_ESTATE.  The current batch, its forward pass and the batch buffers stay as they were (adopt runs the
 * forward pass the batch would get anyway).
 *
 *   create   capacity >= 1 slots, a ring of history >= 0 ids per slot; every slot is reset.  SBR_EINVAL with the reason: a
 *            bidirectional engine (a backwards layer has no state "after p items"), capacity < 1, history < 0.
 *   reset    the named slots (slots NULL: all of them, n ignored) take the CURRENT hid_init / cell_init -- read by a kernel at that
 *            point of the stream --, 0 events and an empty ring.
 *   advance  one event per named slot through every layer: items[r] (and second[r], the second index per step of a model with
 *            n_feat == 2 -- NULL otherwise) is fed to slot slots[r].  One launch per layer (ses_step_kernel, sbr_session.hip: a
 *            row-gathered GEMM on v_mfma_f32_16x16x4_f32 plus the cell) and one commit launch that counts the event and appends
 *            items[r] to the ring.  An output element is one accumulation chain whose order does not depend on the rows that share
 *            the call: a session fed alone and the same session fed among thousands hold the same bits.
 *   replay   a run of events per named slot, applied in order FROM THE SLOT'S KEPT STATE, in one launch: off is a CSR over the n rows
 *            (n + 1 non-decreasing offsets, off[0] == 0), row r feeds items[off[r] .. off[r + 1]) (and second[..], as advance takes
 *            it) to slot slots[r], oldest first.  Exactly advance called once per event: afterwards the slot has events + len events,
 *            its state in every layer (padded units included) holds the very bits len advance calls would have left, its ring the
 *            last min(events + len, history) ids at the places those events have; a row with len == 0 leaves its slot untouched.  No
 *            limit on a row's length, none on n beyond capacity.  ses_replay_kernel (sbr_session.hip) owns a 16-row tile and every
 *            unit tile of every layer per workgroup, with the time loop and the layer loop inside and the step's own tile arithmetic
 *            (one __device__ function serves both kernels); the rows of a call are tiled longest first, a row whose list has ended is
 *            frozen; the states are exchanged through the slot's own two planes, and the same launch counts the events and writes the
 *            rings: sbr_query "session_replay_launches" (the launches the most recent replay on this engine enqueued) is 1.  The
 *            device buffer of a call's events belongs to the pool, grows when a call needs more and is kept (SBR_ENOMEM before
 *            anything is launched); a call that grows it frees the old one first, and hipFree WAITS for the device -- only such a
 *            call (the first one, and one with more events than any before) does not return at once.  THIS, not adopt, is the road for histories longer than max_length and for continuing a kept
 *            state (a returning user's new events, a pool rebuilt from a log, a slot restored with write and caught up).
 *   replay_ranks   (sbr_sessions_replay_ranks) replay that also ranks every event before it is fed -- the online hit rate of the model
 *            being served on a log, or next-item ranks at every event of test sequences of any length, from the arithmetic that
 *            serves.  slots / n / items / second / off and everything replay refuses are replay's, and so is the effect on the pool:
 *            states of every layer (padded units included), event counts and rings hold the very bits replay -- one advance per
 *            event -- leaves.  Row r names slot s = slots[r], which has e0 events when the call arrives; for its event t,
 *            x_t = items[off[r] + t]:  ranks_host[off[r] + t] = the rankable items that stand before x_t in sbr_rank's order (key
 *            descending, ties to the lowest id) among the scores sbr_sessions_rank(s, exclude_mode) would rank at the moment the slot
 *            has e0 + t events, before x_t is fed; -1 when x_t itself is not rankable there (NaN, -inf, excluded by the mode, id >= N;
 *            with n_feat == 2 only `items` is ranked).  n_rankable_host[off[r] + t] = the rankable items at that moment.  Both
 *            [off[n]].  events_before_host [n], may be NULL: e0 of every row, empty rows included.  The exclusion at event t is
 *            rank's at that moment: the last min(e0 + t, kept) ids fed (kept = 1 for _LAST, `history` for _HISTORY), which come
 *            from x_0 .. x_{t-1} and, where t < kept, from the ring as it stood BEFORE the call (kept aside before the first
 *            launch); an id repeated in that window is excluded once.  On the default projection (and the triage one) an
 *            element of the scores is one accumulation chain whose order does not depend on the rows of a launch, so the result
 *            equals, integer for integer, the loop "rank at k = N, find x_t, advance".  Under SBR_FLAG_BF16_PROJECTION the one-pass
 *            kernel chooses its tile by the row count: there the call gives the ranks of the scores that projection gives for the
 *            group of states it projects together, with no bit promise against the loop (as sbr_evaluate_positions).
 *            The call is cut in time into passes: one tracing launch of ses_replay_kernel from the kept state per pass -- the replay
 *            itself, which also writes the top layer's state in front of every event --, then per group of states the projection
 *            and one counting launch (ses_event_rank_kernel, sbr_eval.hip: one streamed pass over the N scores per event, 16-byte
 *            loads when N % 4 == 0).  group_rows > 0: the most (row, event) pairs whose scores the call holds at once (their
 *            states too, unless more rows than that have events: a pass then takes one event of each and projects them in groups);
 *            0: as many as fit 64 MB of scores.  It bounds the ranking scratch and NOTHING else: results and pool bits are the same
 *            for every value.  sbr_query "session_replay_rank_passes": the passes of the most recent call;
 *            "session_event_rank_form": 1 / 2, 16- / 4-byte loads.  Trace, scores and results live in the handle's ranking scratch, the
 *            events in the pool's buffer (replay's caveat about hipFree holds for both).  SBR_EINVAL before anything is launched, the
 *            pool untouched: everything replay refuses, a mode outside the three, group_rows < 0, ranks_host / n_rankable_host NULL
 *            with off[n] > 0, more than 2^31 - 1 events.  SBR_ESTATE as replay.  Lazily stepped rows: the index-input block as
 *            for replay AND the output rows as for rank.  Waits once, at its end.  n == 0 or no events at all: no replay, no
 *            projection, nothing written but events_before (one small launch gathers it when it is asked for).
 *   adopt    the prefill: rows 0 .. n_rows - 1 of the engine's current batch become the sessions slots[0 .. n_rows): the forward
 *            pass runs on the chain kernels (if the batch has none yet), then ONE launch copies each row's state at the row's length
 *            (of every layer), its length as the event count and its last `history` fed ids.  No batch set: SBR_ESTATE.
 *   rank     the next-item ranking of the named slots (they may repeat), n >= 1: the top layer's states are gathered and go through
 *            sbr_rank's own pipeline (projection, exclusion, select, sort) in chunks of local_batch rows.  k, the order, the ties, the
 *            -1 / -inf places, scores_host and the caller's lists excl_ids / excl_off (a CSR over the n rows, excluded IN ADDITION)
 *            are sbr_rank's; ids_host [n][k].  exclude_mode: SBR_SESSION_EXCL_*; with a session longer than `history` only the last
 *            `history` ids are excluded (history == 0: none).
 *   rank_candidates   (sbr_sessions_rank_candidates) rank restricted to a candidate list per named slot: cand_ids / cand_off /
 *            shared, the result, the two forms and their switch are sbr_rank_candidates' (a CSR over the n rows, or one shared list);
 *            slots, chunks, exclude_mode and the caller's lists are rank's.  On the default projection it equals rank at k = N
 *            filtered to the row's list, bit for bit.
 *   read     slot's state in `layer`: h_host / c_host [Hp] floats (Hp = the layer's padded width: 16 / 32 / 64 / 128 / 256 / 512,
 *            above that the next multiple of 64; c_host is written for LSTM only), *events, history_host [history]: the last
 *            min(events, history) ids, oldest first, then -1.  Any output may be NULL.
 *   write    puts h_host (and c_host, LSTM) back as slot's state in `layer`; events and ring stay.  read / write move ONE layer's
 *            state of ONE slot and nothing else (a slot restored with write keeps the event count, the ring and the plane parity of
 *            whoever held it before, and each call waits twice): the hooks for evicting and restoring sessions are export / import.
 *
 * The record of a parked session (record version 1; little-endian, as the machine has it) -- one session off the device:
 *     int64   events
 *     int32   ids[ring_len]     ring_len = max(history, 1): the last min(events, ring_len) ids fed, OLDEST FIRST, then -1
 *             (zeros up to a multiple of 16 bytes)
 *     per layer l = 0 .. L-1:
 *     float   h[Hp_l]           the slot's CURRENT plane (plane events & 1), padded units as the pool keeps them
 *     float   c[Hp_l]           LSTM only
 * record_bytes is a multiple of 16.  The ids stand in canonical order, as read returns them, not as the ring lies in memory, and the
 * record holds no plane parity: it means the same in every slot of every pool of the same layout.  It holds states, not weights: like
 * the pool, it goes on under whatever parameters the engine has.  The layout fingerprint is FNV-1a (64 bit, offset basis
 * 0xcbf29ce484222325, prime 0x100000001b3) over the 32-bit little-endian words (1, cell, L, Hp_0 .. Hp_{L-1}, ring_len).
 *
 *   record_layout   (sbr_sessions_record_layout) record_bytes and the fingerprint for a config and a `history`: pure host code, no
 *            device and no pool (as sbr_arena_bytes).  SBR_EINVAL with the reason: what sbr_create refuses about the config, a
 *            bidirectional config, history < 0.
 *   export   (sbr_sessions_export) the record of slots[r] to records_host + r * record_bytes, n of them (the slots may repeat: the call
 *            only reads the pool).  ses_pack_kernel (sbr_session.hip) reads each slot's event count ON THE DEVICE, takes plane
 *            events & 1 of every layer and puts the ring in canonical order, into the pool's staging buffer; one device-to-host copy
 *            per chunk follows and ONE wait at the end.  cap: the bytes records_host holds; cap < n * record_bytes is SBR_EINVAL.
 *   import   (sbr_sessions_import) the inverse: slot slots[r] (distinct) takes record r -- ses_unpack_kernel sets its event count, writes
 *            h (and c) of every layer to plane events & 1 (the other plane is left alone: nothing reads it before a step writes it)
 *            and rewrites its WHOLE ring: id t of the record at place (events - kept + t) % ring_len, kept = min(events, ring_len),
 *            -1 at every other place.  Nothing of the former occupant survives: afterwards the slot is indistinguishable, through
 *            every call of the pool, from the slot the record was exported from.  Returns when records_host may be reused (pageable
 *            host memory), without waiting for the kernel.  SBR_EINVAL, found on the host before anything is launched, the pool
 *            untouched, the offender named: bytes != n * record_bytes, n above capacity, a slot named twice, events < 0, among the first
 *            `kept` ids one outside [0, input_size), anything but -1 behind them.  The floats are not inspected (as write's are not).
 *   Both run on the engine's stream, return SBR_ESTATE inside an open training step or with a lagged cost pending, and read and write
 *   NOTHING in the arena -- no parameter, no batch buffer, no flush of lazily stepped rows: a training run with parks in it is the run
 *   without them.  n == 0 does nothing.  chunk_slots > 0: the most records staged on the device at once; 0: as many as fit 64 MB;
 *   < 0: SBR_EINVAL.  It bounds the staging buffer and NOTHING else: no byte of the result or of the pool depends on it.  The staging
 *   buffer belongs to the pool, grows when a call needs more and is kept (SBR_ENOMEM before anything is launched; replay's caveat
 *   about hipFree holds).  sbr_query "session_park_chunks": the chunks of the most recent export or import on the engine.
 * SBR_EINVAL, found on the host before anything is launched, the pool untouched, the offender named: a slot outside [0, capacity), a
 * slot named twice in one advance / replay / adopt / reset, an id outside [0, input_size), `second` missing with n_feat == 2 or given
 * with n_feat == 1, n above capacity (advance, replay) or n_rows above the batch's rows (adopt), off not starting at 0 or decreasing, k, exclude_mode or lists as sbr_rank rejects them,
 * candidate lists as sbr_rank_candidates rejects them. */
typedef struct sbr_sessions sbr_sessions;
#define SBR_SESSION_EXCL_NONE    0
#define SBR_SESSION_EXCL_LAST    1   /* the item fed last is not ranked */
#define SBR_SESSION_EXCL_HISTORY 2   /* the kept history (the ring) is not ranked */
int  sbr_sessions_create(sbr_handle* h, int64_t capacity, int32_t history, sbr_sessions** out);
void sbr_sessions_destroy(sbr_sessions* s);            /* before sbr_destroy(h) */
int  sbr_sessions_reset(sbr_sessions* s, const int32_t* slots, int64_t n);
int  sbr_sessions_advance(sbr_sessions* s, const int32_t* slots, const int32_t* items, const int32_t* second, int64_t n);
int  sbr_sessions_replay(sbr_sessions* s, const int32_t* slots, int64_t n,
                         const int32_t* items, const int32_t* second, const int64_t* off);
int  sbr_sessions_replay_ranks(sbr_sessions* s, const int32_t* slots, int64_t n,
                               const int32_t* items, const int32_t* second, const int64_t* off,
                               int exclude_mode, int64_t group_rows,
                               int32_t* ranks_host, int32_t* n_rankable_host, int64_t* events_before_host);
int  sbr_sessions_adopt(sbr_sessions* s, const int32_t* slots, int32_t n_rows);
int  sbr_sessions_rank(sbr_sessions* s, const int32_t* slots, int64_t n, int k, int exclude_mode,
                       const int32_t* excl_ids, const int64_t* excl_off, int32_t* ids_host, float* scores_host);
int  sbr_sessions_rank_candidates(sbr_sessions* s, const int32_t* slots, int64_t n, int k,
                                  const int32_t* cand_ids, const int64_t* cand_off, int shared, int exclude_mode,
                                  const int32_t* excl_ids, const int64_t* excl_off, int32_t* ids_host, float* scores_host);
int  sbr_sessions_read(sbr_sessions* s, int32_t slot, int32_t layer, float* h_host, float* c_host, int64_t* events, int32_t* history_host);
int  sbr_sessions_write(sbr_sessions* s, int32_t slot, int32_t layer, const float* h_host, const float* c_host);
int  sbr_sessions_record_layout(const sbr_config* cfg, int32_t history, size_t* record_bytes, uint64_t* fingerprint);
int  sbr_sessions_export(sbr_sessions* s, const int32_t* slots, int64_t n, int64_t chunk_slots, void* records_host, size_t cap);
int  sbr_sessions_import(sbr_sessions* s, const int32_t* slots, int64_t n, int64_t chunk_slots, const void* records_host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* SBR_RNN_H */
