/* tfrecomm.h - C-ABI of libtfrecomm_hip.so: the MI355X (gfx950) implementation of the
 * SVD matrix-factorisation minibatch training step of jilljenn/TF-recomm.
 *
 * The reference has no native/FFI interface for this path: its boundary is the TensorFlow
 * 1.x Python API.  Each entry point below names the reference call it stands in for
 * (file:line into the reference tree); INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - plain C, no C++ types, no exceptions across the boundary;
 *   - return 0 (TFR_OK) or a negative tfr_status; tfr_last_error() is thread-local text;
 *   - the library owns all device memory; host pointers are borrowed for the duration of
 *     the call and never freed by the library; outputs are caller-allocated;
 *   - one host thread drives one model; work is stream-ordered on the model's HIP stream;
 *     any call with a non-NULL host output pointer synchronises that stream before it
 *     returns; `_dev` entry points take device pointers, return without synchronising
 *     and report id errors at the next synchronising call;
 *   - ids are validated on the device (the reference relies on TensorFlow's CPU gather
 *     raising on out-of-range ids): an out-of-range id makes the step a no-op for every
 *     table and the next synchronising call returns TFR_ERR_OOB;
 *   - there is NO CPU fallback: without a usable HIP device tfr_create fails.
 */
#ifndef TFRECOMM_H
#define TFRECOMM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TFR_ABI_VERSION 3

typedef struct tfr_model tfr_model;

typedef enum {
    TFR_OK = 0,
    TFR_ERR_ARG = -1,     /* bad argument / unsupported shape */
    TFR_ERR_OOB = -2,     /* user or item id outside [0, user_num) / [0, item_num) */
    TFR_ERR_HIP = -3,     /* HIP runtime error (text in tfr_last_error) */
    TFR_ERR_STATE = -4,   /* call not valid in this state (e.g. resident step before upload) */
    TFR_ERR_NOMEM = -5
} tfr_status;

/* which-table ids for set/get/frozen.  Values 0..4 are the five trainables of
 * ops.py:8-12,29-32; +8 / +16 select the Adam first / second moment slot of that table. */
enum {
    TFR_MU = 0,           /* bias_global   []      ops.py:8     */
    TFR_BU = 1,           /* user_bias     [U]     ops.py:9-10  */
    TFR_BI = 2,           /* item_bias     [I]     ops.py:11-12 */
    TFR_P = 3,            /* user_features [U,D]   ops.py:29-30 */
    TFR_Q = 4,            /* item_features [I,D]   ops.py:31-32 */
    TFR_SLOT_M = 8,
    TFR_SLOT_V = 16
};

enum { TFR_LOSS_MSE = 0, TFR_LOSS_NLL = 1 };       /* ops.py:124 (canonical) / ops.py:125-126 (fork) */
enum { TFR_OPT_ADAM = 0, TFR_OPT_SGD = 1 };        /* ops.py:144,148 (canonical) / ops.py:145,149 (fork) */
enum { TFR_ADAM_TF1 = 0, TFR_ADAM_LAZY = 1 };      /* dense-moment TF1 semantics / touched rows only */

typedef struct tfr_opts {
    int32_t loss;         /* TFR_LOSS_*                                                    */
    int32_t item_abs;     /* 1: dot uses |item_features| (ops.py:44)                        */
    int32_t reg_bias;     /* 1: regulariser also has the two bias l2 terms (ops.py:85-89)   */
    int32_t optimizer;    /* TFR_OPT_*                                                     */
    int32_t adam_mode;    /* TFR_ADAM_*                                                    */
    int32_t device;       /* HIP device ordinal                                            */
    float lr;             /* learning_rate (ops.py:118)                                    */
    float reg;            /* reg = lambda  (ops.py:118,137)                                */
    float beta1, beta2, eps;  /* tf.train.AdamOptimizer defaults 0.9, 0.999, 1e-8          */
    int32_t reserved[5];  /* must be zero                                                  */
} tfr_opts;

/* ---- lifetime -------------------------------------------------------------------------- */
/* ops.inference_svd(..., user_num, item_num, dim) variable creation, ops.py:6-12,29-32.
 * Tables start at zero; the host side initialises and uploads them (tfr_set_table). */
int tfr_create(tfr_model** out, int64_t user_num, int64_t item_num, int32_t dim, const tfr_opts* opts);
int tfr_destroy(tfr_model* m);
void tfr_default_opts(tfr_opts* opts);

/* tf.global_variables_initializer() (svd_train_val.py:53,56) on the device: user/item features
 * ~ truncated normal(stddev 0.02), biases ~ truncated normal(stddev 1) (ops.py:9-12,29-32),
 * bias_global ~ U(-sqrt 3, sqrt 3) (TF's default glorot-uniform for a scalar); Adam slots,
 * global_step and the beta powers are reset.  The stream differs from TensorFlow's Philox,
 * so initial values are not a parity target. */
int tfr_init_tables(tfr_model* m, uint64_t seed, float feature_stddev, float bias_stddev);

/* ---- variables: tf.Variable.load / .eval and tf.train.Saver (svd_train_val.py:54,197-198) */
int tfr_set_table(tfr_model* m, int32_t which, const float* host, int64_t n);
int tfr_get_table(tfr_model* m, int32_t which, float* host, int64_t n);
/* var_list of Optimizer.minimize (ops.py:146-149; adaptive_test.py:28): bit (1<<TFR_x) set
 * = table x receives no update. */
int tfr_set_frozen(tfr_model* m, uint32_t mask);
/* global_step (svd_train_val.py:48, ops.py:119-120) and the Adam beta-power accumulators. */
int tfr_get_step(tfr_model* m, int64_t* step, float* beta1_power, float* beta2_power);
int tfr_set_step(tfr_model* m, int64_t step, float beta1_power, float beta2_power);
/* change lr / reg between steps (the reference rebuilds the graph for that; ops.py:118). */
int tfr_set_hyper(tfr_model* m, float lr, float reg);

/* ---- forward: sess.run([logits, infer], feed_dict) - svd_train_val.py:120-122; ops.py:13-14,37-47 */
int tfr_forward(tfr_model* m, const int32_t* user, const int32_t* item, int64_t batch,
                float* logits_out);
/* device-side validation metric: sum_k (infer_k - rate_k)^2 and count of infer==rate
 * (svd_train_val.py:144-149).  host id/rate pointers. */
int tfr_eval(tfr_model* m, const int32_t* user, const int32_t* item, const float* rate,
             int64_t batch, double* sum_sq_err_out, int64_t* n_equal_out);

/* the validation set kept in HBM (svd_train_val.py:33-38 feeds it whole, every epoch):
 * upload once, evaluate with no host data in the loop.  n_out = number of ratings. */
int tfr_upload_eval_triples(tfr_model* m, const int32_t* user, const int32_t* item, const float* rate,
                            int64_t n);
int tfr_eval_resident(tfr_model* m, double* sum_sq_err_out, int64_t* n_equal_out, int64_t* n_out);

/* the fork's epoch metrics on the device (svd_train_val.py:94-98,170-178: per-batch sklearn roc_auc_score and the fed-logits
 * NLL are the host bottleneck SURVEY 8f #1 names): count of round(sigmoid(logit)) == rate, summed sigmoid cross-entropy
 * (ops.py:125-126) and the AUC (rank sum over the radix-sorted logits, equal scores share their mean rank - what
 * roc_auc_score computes; NaN when one class is empty).  Binary-outcome model (loss = nll) only. */
int tfr_eval_binary(tfr_model* m, const int32_t* user, const int32_t* item, const float* rate, int64_t batch,
                    int64_t* n_equal_out, double* nll_sum_out, double* auc_out);
int tfr_eval_binary_resident(tfr_model* m, int64_t* n_equal_out, double* nll_sum_out, double* auc_out, int64_t* n_out);
/* roc_auc_score(rates, sigmoid(logits)) of the batch the last tfr_train_step or tfr_train_steps_repeat ran on (svd_train_val.py:97):
 * its rates against the pre-update logits that call returned (tfr_train_steps_repeat: of its last step).  The batch is kept
 * in the handle's workspace, not copied, so the call is valid only while that batch is still there: after a tfr_train_step /
 * tfr_train_steps_repeat that was given logits_out, of any batch size, and before
 *   - any other training call (the resident, staged, drawn, device-pointer, BPR, fine-tuning, data-parallel and row-sharded
 *     steps, and a tfr_train_step without logits_out),
 *   - tfr_forward, tfr_forward_resident, tfr_eval, tfr_eval_binary[_resident], tfr_bf16_forward, tfr_bf16_eval,
 *   - any call whose batch exceeds the workspace and makes it grow.
 * Each of these forgets the kept batch, and the call then returns TFR_ERR_STATE; it never returns the AUC of other numbers.
 * Calls that leave the batch workspace alone (top-K, ranking, neighbours, the snapshot, get / set of tables, step, frozen
 * mask and hyper-parameters, tfr_eval_resident, tfr_auc_dev and tfr_sort_segments within the capacity, the id draws) keep
 * it; the call itself may be repeated. */
int tfr_last_batch_auc(tfr_model* m, double* auc_out);
/* roc_auc_score(label > 0.5, score) for device arrays */
int tfr_auc_dev(tfr_model* m, const float* d_score, const float* d_label, int64_t n, double* auc_out);

/* ---- one minibatch: sess.run([train_op, logits, infer], feed_dict) - svd_train_val.py:66-72;
 *      ops.py:81-89 (regulariser), ops.py:118-153 (loss, minimize).
 *      logits_out = pre-update logits of this batch; loss_out = data term only
 *      (ops.py:152-153); reg_out = regulariser value.  Any may be NULL. */
int tfr_train_step(tfr_model* m, const int32_t* user, const int32_t* item, const float* rate,
                   int64_t batch, float* logits_out, float* loss_out, float* reg_out);

/* ---- the same minibatch nsteps times: the inner loop of the per-user fine-tuning drivers - adaptive_test.py:104-116
 *      (EPOCH_MAX = 300 x sess.run(train_op) on the asked items of one user) and non_adaptive_test.py:82-87 (100 x on the
 *      user's history), usually with tfr_set_frozen = var_list=[user_bias, user_features] (adaptive_test.py:28).  The batch
 *      is uploaded once and the steps run with no host round trip in between.  logits_out[batch]: pre-update logits of the
 *      LAST step (what the last sess.run would fetch); loss_out[nsteps]: data term per step.  Either may be NULL.  Same
 *      result, bit for bit, as nsteps calls of tfr_train_step. */
int tfr_train_steps_repeat(tfr_model* m, const int32_t* user, const int32_t* item, const float* rate,
                           int64_t batch, int32_t nsteps, float* logits_out, float* loss_out);

/* ---- device-resident (user,item,rate) store: the feed of dataio.ShuffleIterator
 *      (dataio.py:98-103,114-117) kept in HBM; the host still draws the ids. */
int tfr_upload_triples(tfr_model* m, const int32_t* user, const int32_t* item, const float* rate,
                       int64_t n);
/* same, but the three columns are already in HBM (device pointers; copied into the library's
 * own 16-byte-record store, so the caller may free them after the call). */
int tfr_set_triples_dev(tfr_model* m, const int32_t* d_user, const int32_t* d_item,
                        const float* d_rate, int64_t n);
/* ids[step*batch + k] index the store: nsteps minibatches in one call.  loss_out[nsteps]
 * (data term per step) may be NULL (then the call does not synchronise). */
int tfr_train_steps_resident(tfr_model* m, const int64_t* ids, int64_t batch, int32_t nsteps,
                             float* loss_out);
/* upload pre-drawn ids once, then run steps [first, first+nsteps) from them with no host
 * data in the loop. */
int tfr_stage_ids(tfr_model* m, const int64_t* ids, int64_t n);
int tfr_train_steps_staged(tfr_model* m, int64_t first_step, int64_t batch, int32_t nsteps,
                           float* loss_out);
/* ---- the minibatch id draw itself on the device (dataio.py:113-117 `next`): NumPy's legacy global
 *      MT19937 stream (np.random.seed(13575), svd_train_val.py:15) and legacy randint's masked
 *      rejection, replayed bit for bit by one workgroup, so `ids = np.random.randint(0, N, (batch,))`
 *      never touches the host.  The state is what np.random.get_state() holds: key[624] and pos.
 *      high <= 2^32 (NumPy switches to 64-bit draws beyond that). */
int tfr_rng_seed(tfr_model* m, uint32_t seed);                               /* == np.random.seed(seed) */
int tfr_rng_set_state(tfr_model* m, const uint32_t* key624, int32_t pos);    /* np.random.get_state()[1:3] */
int tfr_rng_get_state(tfr_model* m, uint32_t* key624, int32_t* pos);         /* synchronises */
/* ids_out[count] (host) = np.random.randint(0, high, (count,)); advances the device state. */
int tfr_draw_ids(tfr_model* m, int64_t high, int64_t count, int64_t* ids_out);
/* the same draw into DEVICE memory, asynchronously on the draw stream: it starts once everything queued on the model's
 * stream so far has finished (which may still read d_ids_out), and tfr_join_draws makes the model's stream wait for every
 * draw issued so far.  For callers that run the step themselves, one call at a time (the data-parallel loop: every rank
 * draws the global batch's ids - the same stream on every rank - and takes its slice, dataio.py:115 with no host in it). */
int tfr_draw_ids_dev(tfr_model* m, int64_t high, int64_t count, int64_t* d_ids_out);
int tfr_join_draws(tfr_model* m);
/* ...for the first `ordinal` draws only (issued draws are counted from 1 and complete in issue order): a caller that keeps
 * several draws in flight waits for the one whose buffer it is about to read, not for the latest */
int tfr_join_draw(tfr_model* m, int64_t ordinal);
/* nsteps x { next(iter_train); sess.run(train_op) } (svd_train_val.py:66-72) with every part on the
 * device: ids drawn from randint(0, n_store_ratings) as above (on a side stream, ahead of the steps
 * that use them), rows gathered from the resident store, one training step each.  loss_out[nsteps]
 * may be NULL (then the call does not synchronise). */
int tfr_train_steps_drawn(tfr_model* m, int64_t batch, int32_t nsteps, float* loss_out);
/* host-drawn ids (the reference's own np.random.randint call) for ONE step on the resident store:
 * copied into a pinned ring slot, uploaded and trained on asynchronously - returns without waiting;
 * id errors surface at the next synchronising call. */
int tfr_train_step_ids(tfr_model* m, const int64_t* ids, int64_t batch);
/* forward over store rows [lo, hi): logits_out[hi-lo] host, may be NULL */
int tfr_forward_resident(tfr_model* m, int64_t lo, int64_t hi, float* logits_out);

/* ---- device-pointer entry points (plumbing for torch tensors / sharded multi-GPU) ------- */
int tfr_forward_dev(tfr_model* m, const int32_t* d_user, const int32_t* d_item, int64_t batch,
                    float* d_logits);
int tfr_train_step_dev(tfr_model* m, const int32_t* d_user, const int32_t* d_item,
                       const float* d_rate, int64_t batch, float* d_logits /* may be NULL */);
/* (item_features: the fused big-table step keeps updated rows in an alternate table until another reader asks - this call, like
 *  every reader, first brings them back; the pointer is current until the next big-table training step) */
int tfr_table_devptr(tfr_model* m, int32_t which, void** ptr, int64_t* n);
int tfr_set_stream(tfr_model* m, void* hip_stream);   /* NULL = the model's own stream; drains the stream in use first */
/* the same without draining: for a caller that alternates between two streams and orders them itself with events (the
 * row-sharded step prepares batch s+1 on a side stream while step s runs on the main one) */
int tfr_switch_stream(tfr_model* m, void* hip_stream);
int tfr_get_stream(tfr_model* m, void** hip_stream);
/* last step's device scalars {loss, reg, sum_g} without a host copy */
int tfr_scalars_devptr(tfr_model* m, void** ptr);

/* ---- row-sharded building blocks: the same kernels, split so the host can put
 *      an RCCL all-to-all between them.  The handle holds ONE rank's shard (user_num /
 *      item_num = local row counts); bias_global is replicated.  All pointers are device
 *      pointers; calls are asynchronous on the model's stream and NONE of them needs a host
 *      round trip: batch sizes that depend on the data stay on the device, the three exchanges
 *      use fixed-capacity buffers laid out [world][slot_cap] with rows of tfr_shard_row_stride()
 *      floats (dim features, the bias, padding to 16 bytes), so they are equal-split all-to-alls.
 *      Semantics per rank and step (ops.py:143-149 applied to the rows this rank owns):
 *        0. integer routing of the GLOBAL batch (identical on every rank): the samples whose user
 *           row this rank owns (owner = id / ceil(rows / world)), the distinct item ids among them
 *           grouped by owner into request slots (unused slots -1):          tfr_shard_route
 *        1. owners answer row requests:                                      tfr_shard_gather
 *        2. forward + backward on the rank's samples (user rows local, item rows addressed by
 *           slot); user rows are updated in place, item-row gradients (one per slot, already
 *           reduced over this rank's samples) are emitted in the exchange layout:
 *                                                                            tfr_shard_forward_reduce
 *        3. owners add the gradient rows received from all ranks (in rank order) and apply the
 *           optimiser to their item rows:                                    tfr_shard_apply_items
 *        4. with the all-reduced {loss, reg, sum_g}: bias_global update, beta powers,
 *           global_step:                                                     tfr_shard_finish_step
 *      More local samples than sample_cap, or more distinct items for one owner than slot_cap,
 *      void the step like an out-of-range id (TFR_ERR_OOB at the next synchronising call). */
int32_t tfr_shard_row_stride(tfr_model* m);
int tfr_shard_route(tfr_model* m, const int32_t* d_user, const int32_t* d_item, const float* d_rate, int64_t batch_global,
                    int32_t rank, int32_t world, int64_t user_num_global, int64_t item_num_global,
                    int32_t sample_cap, int32_t slot_cap, int32_t* d_req /* out [world * slot_cap] */);
/* the same routing with the global batch given as rows d_ids[0..batch_global) of this rank's copy of the rating store
 * (tfr_upload_triples / tfr_set_triples_dev with GLOBAL user / item ids): the ShuffleIterator gather (dataio.py:115-117)
 * happens inside the routing kernels and only the samples this rank owns leave the store. */
int tfr_shard_route_ids(tfr_model* m, const int64_t* d_ids, int64_t batch_global, int32_t rank, int32_t world,
                        int64_t user_num_global, int64_t item_num_global, int32_t sample_cap, int32_t slot_cap, int32_t* d_req);
/* pre-split batches (SURVEY 8e's other variant): every rank brings only ITS OWN batch rows d_ids[0..batch) of its store copy.
 * tfr_shard_bucket_ids groups their 16-byte records {user, item, rate bits, position} by the owner of the user row into
 * d_send = [world][pair_cap] records (batch order inside a group, unused slots have user = -1; overflow raises the error
 * flag); after one equal-split all-to-all of that buffer tfr_shard_route_recs routes what arrived (n = world * pair_cap
 * records, all owned by this rank) exactly as tfr_shard_route routes a global batch.  No rank ever looks at another rank's
 * samples it does not own: the id draw and the ownership test cost B per rank, not world * B. */
int tfr_shard_bucket_ids(tfr_model* m, const int64_t* d_ids, int64_t batch, int32_t world, int64_t user_num_global,
                         int32_t pair_cap, void* d_send);
int tfr_shard_route_recs(tfr_model* m, const void* d_recs, int64_t n, int32_t rank, int32_t world, int64_t user_num_global,
                         int64_t item_num_global, int32_t sample_cap, int32_t slot_cap, int32_t* d_req);
/* the routed batch, for the caller's bookkeeping and for tests: mine[sample_cap] global batch positions (-1 unused),
 * u_local[sample_cap], slot[sample_cap], counts = {local samples, distinct items, distinct items per owner [world]} */
int tfr_shard_routed_devptrs(tfr_model* m, void** mine, void** u_local, void** slot, void** counts);
int tfr_shard_gather(tfr_model* m, const int32_t* d_req_recv, int64_t n, float* d_rows_out /* [n, stride] */);
int tfr_shard_forward_reduce(tfr_model* m, const float* d_item_rows /* [world * slot_cap, stride] */,
                             float* d_logits /* [sample_cap], may be NULL */, float* d_item_grad /* out, same layout */,
                             float* d_scalars4 /* out: loss, reg, sum_g, - */);
/* the same step in two halves, so that a caller can run the user half BESIDE the gradient exchange (it reads the fetched rows and
 * the local user rows only): tfr_shard_forward_items = sort + forward + item-side reduce into d_item_grad + the local scalars;
 * tfr_shard_reduce_users = user-side reduce + optimiser on the local user rows.  forward_reduce == forward_items; reduce_users. */
int tfr_shard_forward_items(tfr_model* m, const float* d_item_rows, float* d_logits, float* d_item_grad, float* d_scalars4);
int tfr_shard_reduce_users(tfr_model* m, const float* d_item_rows);
int tfr_shard_apply_items(tfr_model* m, const int32_t* d_req_recv, const float* d_grad_recv, int64_t n);
/* Preparing batch s+1 while step s runs.  The model keeps TWO routed-batch sets; tfr_shard_select says which one the route_* calls
 * fill and the forward / reduce / apply calls consume.  tfr_shard_presort does the index work of a step ahead of time on the
 * selected set (it depends on the routed batch and on the requests received, never on a table): the routed samples sorted by
 * local user row and by request slot and - with d_req_recv [n], the requests this rank received as an owner - those requests
 * padded and sorted by item row; the step calls then skip their own sorts.  A caller puts bucket -> exchange -> route_recs ->
 * exchange -> presort of batch s+1 on a side stream (tfr_set_stream) beside step s; every buffer these calls write belongs to
 * the selected set or to the sort scratch, which the step calls then do not touch. */
int tfr_shard_select(tfr_model* m, int32_t which /* 0 or 1 */);
int tfr_shard_presort(tfr_model* m, const int32_t* d_req_recv /* may be NULL */, int64_t n);
int tfr_shard_finish_step(tfr_model* m, const float* d_scalars4 /* global sums */);

/* ---- data-parallel building blocks (replicated tables, small enough that every GPU holds
 *      them): each rank reduces ITS batch to dense gradient buffers, the host all-reduces one
 *      flat buffer (RCCL), every rank applies the same dense update - one `minimize`
 *      (ops.py:143-149) on the union of the ranks' batches.  Needs dense optimiser semantics
 *      (Adam tf1, which is what tf.train.AdamOptimizer computes, or SGD).
 *      d_flat: tfr_dp_flat_size() floats, device memory, zero before the first step:
 *      [user_features grads | item_features grads | user_bias | item_bias | loss, reg, sum_g, 0].
 *      d_store_ids != NULL: the batch is gathered from the resident store (ids index it). */
int64_t tfr_dp_flat_size(tfr_model* m);
int tfr_dp_local_grads(tfr_model* m, const int32_t* d_user, const int32_t* d_item, const float* d_rate,
                       int64_t batch, const int64_t* d_store_ids, float* d_flat);
/* Optional look-ahead for the call above: the store ids (device, same batch size) the NEXT
 * tfr_dp_local_grads will be given.  Their tile sort then rides in this step's launch instead of
 * heading the next step (the host knows the id stream: dataio.py:113-117 draws it).  One-shot. */
int tfr_dp_hint_next(tfr_model* m, const int64_t* d_next_store_ids);
int tfr_dp_apply(tfr_model* m, float* d_flat);
int tfr_staged_ids_devptr(tfr_model* m, void** ptr, int64_t* n);

/* ---- index work of the backward, exposed for bit-exact checks: stable sort of batch
 *      positions by row id (what tf.unique + unsorted_segment_sum's batch-order walk reduce
 *      to).  side 0 = user ids, 1 = item ids.  Host pointers; outputs [batch]. */
int tfr_sort_segments(tfr_model* m, int32_t side, const int32_t* ids, int64_t batch,
                      int32_t* sorted_ids_out, int32_t* sorted_pos_out);

/* ---- FM second-order forward on CSR rows (BASELINE config 5): forward.py:21-22
 *      y(x) = mu + x.W + 0.5 * (||x V||^2 - sum_j x_j^2 ||V_j||^2); design matrix fm.py:61-93.
 *      In the reference the model (mu, W, V) comes from the external libFM binary
 *      (fm.py:154-155, fm_mangaki.py:39-45); here it is uploaded or initialised on the device.
 *      CSR uses scipy.sparse's layout: indptr int64 [n_rows+1], indices int32, data f32. */
typedef struct tfr_fm tfr_fm;
/* opts (NULL = classification / SGD defaults): loss, optimizer (SGD or Adam - always the lazy,
 * touched-rows form), lr, reg, device.  The model is a regular model underneath: V = feature rows,
 * W = their bias column, mu = bias_global. */
int tfr_fm_create(tfr_fm** out, int64_t n_features, int32_t dim, const tfr_opts* opts);
int tfr_fm_destroy(tfr_fm* m);
int tfr_fm_set(tfr_fm* m, float mu, const float* W, const float* V);          /* host pointers */
int tfr_fm_get(tfr_fm* m, float* mu, float* W, float* V);                      /* any may be NULL */
int tfr_fm_init(tfr_fm* m, uint64_t seed, float stddev);                       /* random W, V on device */
/* One table or Adam slot of the FM model: which = TFR_MU, TFR_BU (= W) or TFR_P (= V), optionally or-ed with TFR_SLOT_M /
 * TFR_SLOT_V; n = its element count.  TFR_BI / TFR_Q: TFR_ERR_ARG.  tfr_fm_get_step: as tfr_get_step. */
int tfr_fm_get_table(tfr_fm* m, int32_t which, float* host, int64_t n);
int tfr_fm_get_step(tfr_fm* m, int64_t* step, float* beta1_power, float* beta2_power);
int tfr_fm_forward(tfr_fm* m, const int64_t* indptr, const int32_t* indices, const float* data,
                   int64_t n_rows, float* out);                                /* host CSR, synchronous */
int tfr_fm_forward_dev(tfr_fm* m, const int64_t* d_indptr, const int32_t* d_indices,
                       const float* d_data, int64_t n_rows, float* d_out);     /* device CSR, async */
/* One minibatch of FM training.  NOT a restatement of reference code: the
 * reference trains this model in the external libFM binary by MCMC (fm.py:104-110,154-155).
 * Per non-zero (row r, feature j, x), s_r = x V, g_r = d loss / d y_r:
 *   dV_j += g_r x (s_r - x V_j) + reg V_j;  dW_j += g_r x + reg W_j;  dmu += g_r
 * applied with SGD or lazy Adam; deterministic (sorted segmented reduce, no atomics).
 * pred_out = predictions before the update, loss_out = data loss; either may be NULL. */
int tfr_fm_train_step(tfr_fm* m, const int64_t* indptr, const int32_t* indices, const float* data,
                      const float* y, int64_t n_rows, float* pred_out, float* loss_out);
int tfr_fm_train_step_dev(tfr_fm* m, const int64_t* d_indptr, const int32_t* d_indices,
                          const float* d_data, const float* d_y, int64_t n_rows, int64_t nnz,
                          float* d_pred /* may be NULL */);
int tfr_fm_sync(tfr_fm* m, float* last_kernel_ms);
const char* tfr_fm_last_error(void);

/* ---- FM trainer: resident rows, minibatches gathered on the device, metrics (fm.py:113-131 without host data in the loop)
 *      tfr_fm_upload_rows copies a host CSR (scipy layout) and its targets once into buffers the handle owns; which = 0 is
 *      the train store, 1 the eval store; a second upload replaces the first.  Checked on the host before any device work:
 *      indptr starts at 0 and is non-decreasing (TFR_ERR_ARG), feature ids lie in [0, n_features) (TFR_ERR_OOB).  The call
 *      synchronises.  The handle keeps the row lengths on the host: a step's radix sort and segmented reduce are launched
 *      with a host-side nnz, which is then a sum over the step's ids and not a read-back. */
int tfr_fm_upload_rows(tfr_fm* m, int32_t which, const int64_t* indptr, const int32_t* indices, const float* data,
                       const float* y, int64_t n_rows);
/* nsteps minibatches of `batch` train-store rows each: step s trains on rows ids[s*batch .. (s+1)*batch) - scipy's X[ids],
 * y[ids]: rows in id order, duplicates repeated, empty rows empty - gathered on the device into the handle's minibatch
 * buffers, then the step of tfr_fm_train_step.  Tables, Adam slots, step counter, beta powers and loss_out[s] are bit for bit
 * those of nsteps tfr_fm_train_step calls on the same rows.  ids are host values, checked against [0, n_rows) before
 * anything is queued (TFR_ERR_OOB: no work is done, the model is untouched) and uploaded once.  A batch of empty rows
 * (nnz 0) is a valid step.  loss_out [nsteps] may be NULL: the call then returns with the steps queued (tfr_fm_sync waits).
 * A failure to queue a step, or (with loss_out) an error the device reports, restores the step counter and the beta powers
 * of before the call; steps that ran before it have written their rows, so upload the tables again (tfr_fm_set) before
 * going on.  With loss_out NULL a device error shows at the next synchronising call, which cannot restore this call's
 * counter.  No train store: TFR_ERR_STATE. */
int tfr_fm_train_steps_resident(tfr_fm* m, const int64_t* ids, int64_t batch, int32_t nsteps, float* loss_out);
/* The minibatch tfr_fm_train_steps_resident builds for `ids`, copied to the host: indptr_out [batch + 1], y_out [batch],
 * indices_out / data_out [nnz_cap].  More entries than nnz_cap: TFR_ERR_ARG before any device work.  Synchronous. */
int tfr_fm_gather_rows(tfr_fm* m, int32_t which, const int64_t* ids, int64_t batch, int64_t* indptr_out,
                       int32_t* indices_out, float* data_out, float* y_out, int64_t nnz_cap);
/* Predictions (forward.py:21-22) of every row of a store into out [n_rows] (host).  Synchronous. */
int tfr_fm_predict_resident(tfr_fm* m, int32_t which, float* out);
/* tfr_eval_binary_resident for the FM, over the eval store: the count of round(sigmoid(pred)) == y, the summed sigmoid
 * cross-entropy, the rank-sum AUC (ties share their mean rank; NaN when a class is empty; targets > 0.5 are positives) and
 * the row count.  Needs loss = nll (TFR_ERR_STATE otherwise, and without an eval store).  Outputs may be NULL. */
int tfr_fm_eval_binary_resident(tfr_fm* m, int64_t* n_equal_out, double* nll_sum_out, double* auc_out, int64_t* n_out);

/* ---- ALS baseline (als3.py), float64 like the reference ----------------------
 *      MangakiALS3.fit (als3.py:20-35) = tfr_als_set (init_vars, als3.py:57-65, drawn by the host
 *      from np.random.rand) + tfr_als_load (bias = mean(y); per-user / per-work rating lists,
 *      als3.py:36-55) + tfr_als_sweep (fit_user / fit_work for every user then every work,
 *      als3.py:67-108); predict = tfr_als_predict at explicit pairs (als3.py:110-113).
 *      nb_components <= 32.  Host pointers; calls synchronise. */
typedef struct tfr_als tfr_als;
int tfr_als_create(tfr_als** out, int64_t nb_users, int64_t nb_works, int32_t nb_components,
                   double lambda_, int32_t device);
int tfr_als_destroy(tfr_als* m);
int tfr_als_set(tfr_als* m, const double* U, const double* V, const double* W_user, const double* W_work);
int tfr_als_get(tfr_als* m, double* U, double* V, double* W_user, double* W_work, double* bias);
int tfr_als_set_bias(tfr_als* m, double bias);
int tfr_als_load(tfr_als* m, const int64_t* user_ids, const int64_t* work_ids, const double* y, int64_t n);
int tfr_als_sweep(tfr_als* m, int32_t n_iterations, float* elapsed_ms /* may be NULL */);
int tfr_als_predict(tfr_als* m, const int64_t* user_ids, const int64_t* work_ids, int64_t n, double* out);
const char* tfr_als_last_error(void);

/* ---- implicit-feedback ALS (Hu, Koren, Volinsky: weighted matrix factorisation), float64, 1 <= d <= 64 ----------------
 *      Data: a user x item CSR R of strictly positive values, each row strictly increasing in item id.  Preference
 *      p_ui = 1 on stored pairs, 0 elsewhere; confidence c_ui = 1 + alpha r_ui on stored pairs, 1 elsewhere.  Minimises
 *          L(X, Y) = sum_{u,i} c_ui (p_ui - x_u . y_i)^2 + lambda (||X||_F^2 + ||Y||_F^2)       over all U x I pairs.
 *      A half-sweep of side 0 solves, for every user, (G + sum_{i in N(u)} (c_ui - 1) y_i y_i^T + lambda I) x_u =
 *      sum_{i in N(u)} c_ui y_i with G = Y^T Y (Cholesky); a user without pairs gets exactly 0.  Side 1 is the same for the
 *      items over the transposed lists (users ascending), which tfr_ials_load builds.  tfr_ials_sweep runs n x (side 0,
 *      side 1).  Every sum has a fixed order (32-row tiles, chunks of `chunk` entries for longer lists, Gram slices set by
 *      the table's row count alone): results are bit-identical from run to run.
 *      tfr_ials_gram(side) returns T^T T of side's table: what the next half-sweep of the OTHER side uses.
 *      tfr_ials_loss evaluates L without the dense matrix: sum_u [x_u^T G x_u + sum_{N(u)} (c (1 - s)^2 - s^2)] +
 *      lambda (||X||^2 + trace G), s = x_u . y_i, G = Y^T Y.
 *      Host pointers; every call synchronises.  Checked before any device work (the model is left as it was):
 *      TFR_ERR_ARG for d outside [1, 64], lambda_ <= 0, alpha < 0, a value that is not positive and finite, a row that is
 *      not strictly increasing, a chunk that is not a positive multiple of 32 (0 = 512); TFR_ERR_OOB for an item id out
 *      of range; TFR_ERR_STATE for half, sweep or loss before a load.  A second load replaces the first. */
typedef struct tfr_ials tfr_ials;
int tfr_ials_create(tfr_ials** out, int64_t n_users, int64_t n_items, int32_t d, double lambda_, double alpha, int32_t device);
int tfr_ials_destroy(tfr_ials* m);
int tfr_ials_set(tfr_ials* m, const double* X, const double* Y);          /* either may be NULL */
int tfr_ials_get(tfr_ials* m, double* X, double* Y);                      /* either may be NULL */
int tfr_ials_load(tfr_ials* m, const int64_t* indptr /* [n_users+1] */, const int32_t* items, const double* vals,
                  int32_t chunk /* 0 = 512 */);
int tfr_ials_half(tfr_ials* m, int32_t side /* 0 users, 1 items */, float* elapsed_ms /* may be NULL */);
int tfr_ials_sweep(tfr_ials* m, int32_t n_iterations, float* elapsed_ms /* may be NULL */);
int tfr_ials_gram(tfr_ials* m, int32_t side, double* G_out /* [d*d] */);
int tfr_ials_loss(tfr_ials* m, double* loss_out);
const char* tfr_ials_last_error(void);

/* ---- implicit-feedback ALS by conjugate gradient: the model and loss of the block above, float64, 1 <= d <= 256 ----------
 *      tfr_ials_create_cg makes the same handle type; set, get, load, half, sweep, gram, loss and destroy work on it at any
 *      d <= 256, and half and sweep run the solver below instead of the Cholesky solve.  No per-row matrix is formed.
 *      A half-sweep of side 0 uses G = Y^T Y, computed once per half-sweep.  For each user with list N(u) in CSR order,
 *      w_i = alpha r_ui, c_i = 1 + w_i:
 *          x  = X[u]                                             warm start: the row as it stands
 *          r  = sum_{i in N(u)} (c_i - w_i (y_i . x)) y_i - (G x + lambda x)
 *          p  = r ;  rs = r . r ;  stop = 2^-104 rs
 *          repeat at most cg_steps times, while rs > stop:
 *              Ap = G p + lambda p + sum_{i in N(u)} w_i (y_i . p) y_i
 *              a  = rs / (p . Ap) ;  x += a p ;  r -= a Ap
 *              rn = r . r ;  p = r + (rn / rs) p ;  rs = rn
 *          X[u] = x
 *      A user without pairs gets exactly 0 (the minimiser, and what the Cholesky path writes).  Side 1 is the same over the
 *      transposed lists.  rs > stop is the only early exit: it is false when r is exactly 0 and once the residual has
 *      dropped to the rounding level of its start, where a further step would divide rounding noise by rounding noise.
 *      Every sum has a fixed order that depends on d and the list alone (list entry k and row k of G go to wave k mod 4 of
 *      the row's block, the four waves' vectors are added in wave order; the Gram's slices as above, its output cut into
 *      64 x 64 tiles, G bitwise symmetric): results are bit-identical from run to run.  tfr_ials_load checks `chunk` as
 *      above; this path does not use it.
 *      TFR_ERR_ARG before any device work (*out stays NULL) for d outside [1, 256], cg_steps outside [1, 1024], lambda_ <= 0
 *      or alpha < 0. */
int tfr_ials_create_cg(tfr_ials** out, int64_t n_users, int64_t n_items, int32_t d, double lambda_, double alpha,
                       int32_t cg_steps, int32_t device);

/* ---- implicit-feedback ALS: folding new users and items into fitted factors, on a handle of either solver ----------------
 *      tfr_ials_fold_in solves, for each of n lists (a CSR of partner ids and positive values: items for side 0, users for
 *      side 1, each list strictly increasing), the row a half-sweep of `side` would give an entity holding that list, from the
 *      partner table as it stands and the model's lambda, alpha and solver.  It runs the half-sweep's kernels on these lists
 *      (chunks of `chunk` entries for longer lists on the Cholesky path): for a list the model holds, loaded at the same chunk,
 *      the row has the bits tfr_ials_half would write.  An empty list gives exactly 0; n = 0 is a no-op.  It needs factors,
 *      not a load.
 *      Cholesky handle: the half-sweep's system.  Conjugate-gradient handle: cg_steps steps from start[e] when `start` is
 *      given, else from row rows[e] of side's table as it stands when `rows` is given, else from 0.
 *      The rows stay in a device buffer of the handle until the next fold-in (tfr_ials_export_f32, which = 2); they are
 *      copied to `out` when given and written into rows rows[e] of side's table when `rows` is given.  The resident lists
 *      and their chunk plans are never changed: a later sweep uses what tfr_ials_load gave it.
 *      The Gram of the partner table is computed only when the handle's Gram is not already that table's: the handle
 *      remembers which table its Gram was taken of and forgets it whenever that table may have changed (tfr_ials_set of it,
 *      a half-sweep of its side, a fold-in with `rows` into it).  The Gram is deterministic, so the rows do not depend on
 *      which case applied.
 *      Checked before any device work (tables, resident lists and chunk plans are left as they were): TFR_ERR_ARG for a bad
 *      side, a null indptr, an indptr that does not start at 0 or decreases, a list that is not strictly increasing, a value
 *      that is not positive and finite, a chunk that is not a positive multiple of 32 (0 = 512), duplicate or negative
 *      `rows`, `start` on a Cholesky handle; TFR_ERR_OOB for a partner id or a `rows` entry out of range.
 *      tfr_ials_export_f32 writes rows [row_lo, row_lo + n_rows) of X (which = 0), Y (1) or the last fold-in (2) as float32,
 *      rounded to nearest even, into the caller's DEVICE buffer d_dst [n_rows, d]: the device form of the cast a serving
 *      table needs.  TFR_ERR_ARG for a window outside the table or outside the last fold-in, TFR_ERR_STATE for which = 2
 *      before any fold-in.  Host pointers except d_dst; both calls synchronise. */
int tfr_ials_fold_in(tfr_ials* m, int32_t side /* 0: new users from item lists; 1: new items from user lists */,
                     int64_t n, const int64_t* indptr /* [n+1] */, const int32_t* ids, const double* vals,
                     int32_t chunk /* 0 = 512 */,
                     const int32_t* rows  /* NULL, or [n] distinct rows of side's table: results are written there */,
                     const double* start  /* NULL, or [n, d]: conjugate-gradient handles only */,
                     double* out          /* NULL, or [n, d] host */,
                     float* elapsed_ms    /* may be NULL */);
int tfr_ials_export_f32(tfr_ials* m, int32_t which /* 0 X, 1 Y, 2 the rows of the last fold-in */,
                        int64_t row_lo, int64_t n_rows, void* d_dst /* device, float [n_rows, d] */);

/* ---- top-K recommendation: forward.py:47-61 get_ranking(), als3.py:110-113 (rank the dense U.V^T + biases) ----------------
 *      score(u, i) = ((dot + mu) + bu[u]) + bi[i] (the forward's order), dot = the f32 fmaf chain over f = 0..dim-1 ascending,
 *      from +0, of P[u,f] * Q'[i,f] (Q' = |Q| with item_abs); the logit under the NLL head.  Per requested user the k best
 *      items by score descending, then item id ascending; NaN scores are never returned; slots past the eligible items hold
 *      item -1 / score -INFINITY.  1 <= k <= 256; duplicate users allowed; n_users = 0 is a no-op.
 *      Exclusions: optional CSR (excl_indptr [n_users+1], excl_items) aligned with `users`, each row non-decreasing: items
 *      never returned for that row.  The host entries check ids and order first (TFR_ERR_OOB for an id out of range,
 *      TFR_ERR_ARG for an unsorted row; outputs untouched); tfr_topk_dev checks on the device and reports through the next
 *      synchronising call (its outputs are then unspecified).  Reads the five tables only; runs on the model's stream; the
 *      host entries synchronise, tfr_topk_dev does not.  scores_out may be NULL. */
int tfr_topk(tfr_model* m, const int32_t* users, int64_t n_users, int32_t k,
             const int64_t* excl_indptr /* [n_users+1] or NULL */, const int32_t* excl_items,
             int32_t* items_out /* [n_users,k] */, float* scores_out /* [n_users,k], may be NULL */);
int tfr_topk_dev(tfr_model* m, const int32_t* d_users, int64_t n_users, int32_t k,
                 const int64_t* d_excl_indptr, const int32_t* d_excl_items,
                 int32_t* d_items_out, float* d_scores_out);
/* FM (tfr_fm): user feature u against item features j in [item_lo, item_hi): ((dot(V[u], V[j]) + mu) + W[u]) + W[j] - forward.py
 * on the two-hot row e_u + e_j.  Item ids (returned and excluded) are relative to item_lo. */
int tfr_fm_topk(tfr_fm* m, const int32_t* user_features, int64_t n_users, int64_t item_lo, int64_t item_hi,
                int32_t k, const int64_t* excl_indptr, const int32_t* excl_items /* relative to item_lo */,
                int32_t* items_out, float* scores_out);
/* host-only, no device: what the launcher will do for this shape - LDS bytes per workgroup (the larger of the scoring and the
 * merge kernel), users per scoring workgroup, item slices, users per chunk */
int tfr_topk_plan(int32_t dim, int32_t k, int64_t n_users, int64_t item_num,
                  int64_t* lds_bytes, int32_t* users_per_block, int32_t* item_slices, int64_t* user_chunk);

/* ---- held-out ranking over the whole catalogue: the ranking form of the reference's AUC (svd_train_val.py:97,141,
 *      non_adaptive_test.py:121, fm.py:164) - DESIGN §13 ---------------------------------------------------------------------
 *      Row r ranks the target items T = tgt_items[tgt_indptr[r], tgt_indptr[r+1]) (strictly increasing) of user u = users[r]
 *      among the eligible items E = [0, n_items) minus the row's exclusions X (optional CSR aligned with users, rows
 *      non-decreasing, as tfr_topk).  key(u, i) = the tfr_topk key: the order-preserving uint32 of
 *      score = ((dot + mu) + bu[u]) + bi[i] (dot the f32 fmaf chain over f ascending from +0, |Q| under item_abs), then ~i.
 *          rank(t) = #{ i in E : score(u,i) not NaN and key(u,i) > key(u,t) }   if t in E and score(u,t) is not NaN
 *          rank(t) = -1                                                           otherwise (unranked)
 *      0-based, counting the other targets, distinct within a row (ties by item id).  For every K <= 256, 0 <= rank(t) < K
 *      exactly when t is in tfr_topk(users, K, X)[r], and rank(t) is its position there.  Integer counts: bit-identical
 *      run to run and whatever the batch, duplicates, chunking, slicing and row order.
 *      ranks_out[e - tgt_indptr[0]] = rank of tgt_items[e].  Ids and the CSR shapes are checked on the host before any
 *      device work (TFR_ERR_OOB for an id out of range, TFR_ERR_ARG otherwise; ranks_out untouched).  n_users = 0 and rows
 *      without targets are no-ops.  Reads the five tables only; runs on the model's stream and synchronises. */
int tfr_rank_items(tfr_model* m, const int32_t* users, int64_t n_users,
                   const int64_t* tgt_indptr /* [n_users+1] */, const int32_t* tgt_items,
                   const int64_t* excl_indptr /* [n_users+1] or NULL */, const int32_t* excl_items,
                   int32_t* ranks_out /* [tgt_indptr[n_users] - tgt_indptr[0]] */);
/* FM (tfr_fm): the tables of tfr_fm_topk; target and excluded ids relative to item_lo. */
int tfr_fm_rank_items(tfr_fm* m, const int32_t* user_features, int64_t n_users, int64_t item_lo, int64_t item_hi,
                      const int64_t* tgt_indptr, const int32_t* tgt_items, const int64_t* excl_indptr,
                      const int32_t* excl_items, int32_t* ranks_out);
/* host-only, no device: what the launcher will do for n_users rows holding n_targets targets in all (at most
 * min(n_targets, n_users + n_targets / targets_per_piece) pieces) - LDS bytes per workgroup (the larger of the target and
 * the counting kernel), pieces per counting workgroup, item slices, targets per piece, pieces per chunk */
int tfr_rank_plan(int32_t dim, int64_t n_users, int64_t n_targets, int64_t item_num, int64_t* lds_bytes,
                  int32_t* pieces_per_block, int32_t* item_slices, int32_t* targets_per_piece, int64_t* piece_chunk);

/* ---- item-based nearest neighbours (ItemKNN) from the interaction matrix itself - DESIGN §31 ---------------------------------
 *      X: the binary user x item matrix, a CSR pattern [n_users, n_items] with strictly increasing rows (no values).
 *      n_i = the users of item i, c_ij = the users who have both i and j.  Similarity, in float64 with IEEE operations from
 *      the three integers and rounded once to float32:
 *          metric 0 cosine   c / (sqrt((double)n_i * (double)n_j) + shrink)
 *          metric 1 jaccard  c / ((double)(n_i + n_j - c) + shrink)
 *          metric 2 count    (double)c                                      (shrink must be 0)
 *      The neighbours of i: the K items j != i with c_ij > 0 that have the largest tfr_topk key (the order-preserving uint32
 *      of the similarity, then ~j: similarity descending, then id ascending); rows with fewer are padded with item -1 /
 *      score -INFINITY as tfr_topk pads.  1 <= K <= 256.  Counts are integers: the lists are bit-identical run to run.
 *          score(u, j) = sum over i in N(u), i ascending, of s(i -> j)     s(i -> j) = the float32 similarity when j is
 *      among i's K kept neighbours.  A float32 add chain from +0.  Every item of the catalogue is a candidate; one without
 *      evidence scores exactly 0 and is ordered by id like any tie.  tfr_knn_topk / tfr_knn_topk_lists / tfr_knn_rank_items
 *      are tfr_topk / tfr_rank_items on these scores, word for word: 1 <= k <= 256, exclusion CSR aligned with the queries
 *      with non-decreasing rows, the key, the padding, -1 for an excluded target, target rows strictly increasing, duplicate
 *      users allowed, and 0 <= rank < k exactly when tfr_knn_topk(k) returns the target, at that position.
 *      tfr_knn_load takes the user CSR and builds its transpose; a second load replaces the first and forgets the fitted
 *      lists.  tfr_knn_fit computes the [n_items, K] lists, which stay on the device.  tfr_knn_get_neighbours copies rows
 *      [row_lo, row_lo + n_rows) out; tfr_knn_set_neighbours writes them from host arrays of the same shape (a fitted model
 *      reloaded without a fit; rows never written are empty): ids in [-1, n_items), -1 is padding, no row lists itself or
 *      repeats an item, the scores of real ids are finite.  tfr_knn_topk queries resident users (their loaded rows are the
 *      lists); tfr_knn_topk_lists queries n given lists (a CSR from 0 with strictly increasing rows): users the model does
 *      not hold.  It needs lists, not a load.
 *      Host pointers; every call synchronises.  Checked on the host before any device work (the model is left as it was):
 *      TFR_ERR_ARG for K or k outside [1, 256], an unknown metric, a shrink that is negative or not finite, a shrink with
 *      metric 2, a catalogue of more than 16384 * min(256, 8192 / K) items (fit) or 8192 * min(256, 8192 / k) items (top-K:
 *      the slices the merge takes, tfr_knn_plan), an indptr that
 *      does not start at 0 (user and list CSR) or decreases, a row out of order, a set_neighbours row that lists itself,
 *      repeats an item or carries a score that is not finite; TFR_ERR_OOB for an id out of range; TFR_ERR_STATE for fit
 *      before a load, and for get_neighbours, top-K and ranking before a fit or set_neighbours (top-K of users and ranking
 *      also before a load).  n = 0 and rows without targets are no-ops.  scores_out may be NULL. */
typedef struct tfr_knn tfr_knn;
int tfr_knn_create(tfr_knn** out, int64_t n_users, int64_t n_items, int32_t K, int32_t metric /* 0 cosine, 1 jaccard, 2 count */,
                   double shrink, int32_t device);
int tfr_knn_destroy(tfr_knn* m);
int tfr_knn_load(tfr_knn* m, const int64_t* indptr /* [n_users+1] */, const int32_t* items);
int tfr_knn_fit(tfr_knn* m, float* elapsed_ms /* may be NULL */);
int tfr_knn_get_neighbours(tfr_knn* m, int64_t row_lo, int64_t n_rows, int32_t* items_out /* [n_rows,K], may be NULL */,
                           float* scores_out /* [n_rows,K], may be NULL */);
int tfr_knn_set_neighbours(tfr_knn* m, int64_t row_lo, int64_t n_rows, const int32_t* items, const float* scores);
int tfr_knn_topk(tfr_knn* m, const int32_t* users, int64_t n, int32_t k,
                 const int64_t* excl_indptr /* [n+1] or NULL */, const int32_t* excl_items,
                 int32_t* items_out /* [n,k] */, float* scores_out /* [n,k], may be NULL */);
int tfr_knn_topk_lists(tfr_knn* m, const int64_t* list_indptr /* [n+1] */, const int32_t* list_items, int64_t n, int32_t k,
                       const int64_t* excl_indptr /* [n+1] or NULL */, const int32_t* excl_items,
                       int32_t* items_out, float* scores_out);
int tfr_knn_rank_items(tfr_knn* m, const int32_t* users, int64_t n,
                       const int64_t* tgt_indptr /* [n+1] */, const int32_t* tgt_items,
                       const int64_t* excl_indptr /* [n+1] or NULL */, const int32_t* excl_items,
                       int32_t* ranks_out /* [tgt_indptr[n] - tgt_indptr[0]] */);
/* host-only, no device: what the launcher of the fit (which = 0: k is K, n_rows the items) or of the scoring (which = 1: k is
 * the query's k, n_rows the queries) will do - columns per catalogue slice, slices, rows per chunk, LDS bytes per workgroup
 * (the larger of that kernel and the merge), and how many list entries a wave loads ahead (fit: users of the item whose
 * row bounds are fetched at once; scoring: items of the query whose neighbour rows are).  Outputs may be NULL. */
int tfr_knn_plan(int64_t n_items, int32_t k, int64_t n_rows, int32_t which, int32_t* slice_width, int32_t* slices,
                 int64_t* row_chunk, int64_t* lds_bytes, int32_t* look_ahead);
/* ---- weighted co-occurrence fit on the same handle (RP3beta, P3alpha, TF-IDF / BM25 neighbours on binary data) - DESIGN §35 --
 *      X as loaded; N(i) = the users of item i.  The caller gives q[u], a uint64 weight per user; row_scale[i] and
 *      col_scale[j], a float64 per item, finite and >= 0; and shift, an integer in [0, 62].
 *          S_ij = sum of q[u] over u in N(i) and N(j)                        an exact integer below 2^63
 *          sim(i -> j) = (float)(((double)S_ij * 2^-shift) * row_scale[i] * col_scale[j])
 *      (double)S_ij is correctly rounded, the scaling by a power of two is exact, the two float64 products go left to right,
 *      and there is one rounding to float32; there is no add, so nothing contracts into an fma.  The neighbours of i are
 *      the K items j != i with S_ij > 0 - whatever float32 the similarity rounds to, +0 included - that have the largest
 *      tfr_topk key; padding is item -1 / score -INFINITY as tfr_knn_fit writes it.  The diagonal is left out by
 *      definition.  A user with q[u] = 0 contributes nothing.  Integer sums: the lists are bit-identical run to run.
 *      RP3beta (Paudel et al. 2017) with user weights rounded to multiples of 2^-shift:
 *          q[u] = rint(deg(u)^-alpha * 2^shift), row_scale[i] = n_i^-alpha, col_scale[j] = n_j^-beta, 0 for empty users
 *      and items; beta = 0 is P3alpha (Cooper et al. 2014).  The Python classes RP3beta / WeightedItemKNN build these in
 *      NumPy float64.  The metric and shrink given at create play no part.  The lists replace those of tfr_knn_fit and
 *      are served, read and written by the same entries.
 *      Checked on the host before any device work (the model is left as it was): TFR_ERR_ARG for a NULL handle or array,
 *      a shift outside [0, 62], a scale that is negative or not finite, max q[u] * (the longest loaded item list) not
 *      below 2^63, that product * 2^-shift * max row_scale * max col_scale past FLT_MAX (so every kept similarity is
 *      finite), a catalogue of more than 8192 * min(256, 8192 / K) items (tfr_knn_weighted_plan); TFR_ERR_STATE before a
 *      load.  tfr_knn_weighted_plan is tfr_knn_plan's which = 0 for this fit: host-only, outputs may be NULL. */
int tfr_knn_fit_weighted(tfr_knn* m, const uint64_t* user_w /* [n_users] */, const double* row_scale /* [n_items] */,
                         const double* col_scale /* [n_items] */, int32_t shift, float* elapsed_ms /* may be NULL */);
int tfr_knn_weighted_plan(int64_t n_items, int32_t k, int64_t n_rows, int32_t* slice_width, int32_t* slices,
                          int64_t* row_chunk, int64_t* lds_bytes, int32_t* look_ahead);
const char* tfr_knn_last_error(void);

/* ---- user-based nearest neighbours (UserKNN) from the same interaction matrix - DESIGN §36 -----------------------------------
 *      X: the binary user x item matrix, a CSR pattern [n_users, n_items] under the rules of tfr_knn_load (rows strictly
 *      increasing, no values).  d_u = the items of user u, c_uv = the items both u and v have.  sim(u -> v) comes from the
 *      three integers (c_uv, d_u, d_v) exactly as tfr_knn's similarity comes from (c_ij, n_i, n_j): metric 0 cosine, 1 jaccard,
 *      2 count, in float64 with IEEE operations, rounded once to float32; the rules for shrink are the same.
 *      The neighbours of u: the K users v != u with c_uv > 0 that have the largest tfr_topk key (similarity descending, then
 *      id ascending); rows with fewer are padded with user -1 / score -INFINITY.  1 <= K <= 256.  Counts are integers: the
 *      lists are bit-identical run to run.
 *          score(u, j) = sum over u's kept neighbours v in list order, slot 0 first, of s(u -> v) for the v with j in N(v)
 *      A float32 add chain from +0.  Every item of the catalogue is a candidate; one without evidence scores exactly +0 and
 *      is ordered by id like any tie.  The sum is NOT divided by the sum of the similarities: a constant per user moves no
 *      ranking, and without it the chain is a pure sum of stored float32 values.
 *      tfr_uknn_topk / tfr_uknn_topk_lists / tfr_uknn_rank_items are tfr_topk / tfr_rank_items on these scores, word for word
 *      as their tfr_knn_* namesakes: 1 <= k <= 256, exclusion CSR aligned with the queries with non-decreasing rows, the key,
 *      the padding, -1 for an excluded target, target rows strictly increasing, duplicate users allowed, a NaN score never
 *      returned and never ranked, and 0 <= rank < k exactly when tfr_uknn_topk(k) returns the target, at that position.
 *      tfr_uknn_load takes the user CSR and builds its transpose; a second load replaces the first and forgets the lists.
 *      tfr_uknn_fit computes the [n_users, K] lists, which stay on the device.  tfr_uknn_get_neighbours copies rows
 *      [row_lo, row_lo + n_rows) out; tfr_uknn_set_neighbours writes them from host arrays of the same shape (rows never
 *      written are empty): ids in [-1, n_users), -1 is padding, no row lists itself or repeats a user, the scores of real ids
 *      are finite.  tfr_uknn_topk and tfr_uknn_rank_items query resident users through their lists.
 *      tfr_uknn_topk_lists queries n users known only by a list L (a CSR from 0 with strictly increasing rows): the neighbours
 *      of L are the K resident users v with |L n N(v)| > 0 and the largest key of sim computed from (|L n N(v)|, |L|, d_v).
 *      Nothing is left out as "self": a resident user whose row equals L is simply its best neighbour.  The score is the
 *      same chain over these neighbours.  This entry needs a load, not a fit, and ignores fitted or set lists.
 *      Host pointers; every call synchronises.  Checked on the host before any device work (the model is left as it was):
 *      TFR_ERR_ARG for K or k outside [1, 256], an unknown metric, a shrink that is negative or not finite, a shrink with
 *      metric 2, more than 16384 * min(256, 8192 / K) users (create: the fit and the list search), a catalogue of more than
 *      8192 * min(256, 8192 / k) items (top-K; tfr_uknn_plan), an indptr that does not start at 0 (user and list CSR) or
 *      decreases, a row out of order, a window outside the n_users rows, a set_neighbours row that lists itself, repeats a
 *      user or carries a score that is not finite; TFR_ERR_OOB for an id out of range; TFR_ERR_STATE for fit and top-K of
 *      lists before a load, and for get_neighbours, top-K and ranking before a fit or set_neighbours (those two also before a
 *      load).  n = 0 and rows without targets are no-ops.  scores_out may be NULL. */
typedef struct tfr_uknn tfr_uknn;
int tfr_uknn_create(tfr_uknn** out, int64_t n_users, int64_t n_items, int32_t K, int32_t metric /* 0 cosine, 1 jaccard, 2 count */,
                    double shrink, int32_t device);
int tfr_uknn_destroy(tfr_uknn* m);
int tfr_uknn_load(tfr_uknn* m, const int64_t* indptr /* [n_users+1] */, const int32_t* items);
int tfr_uknn_fit(tfr_uknn* m, float* elapsed_ms /* may be NULL */);
int tfr_uknn_get_neighbours(tfr_uknn* m, int64_t row_lo, int64_t n_rows, int32_t* users_out /* [n_rows,K], may be NULL */,
                            float* scores_out /* [n_rows,K], may be NULL */);
int tfr_uknn_set_neighbours(tfr_uknn* m, int64_t row_lo, int64_t n_rows, const int32_t* users, const float* scores);
int tfr_uknn_topk(tfr_uknn* m, const int32_t* users, int64_t n, int32_t k,
                  const int64_t* excl_indptr /* [n+1] or NULL */, const int32_t* excl_items,
                  int32_t* items_out /* [n,k] */, float* scores_out /* [n,k], may be NULL */);
int tfr_uknn_topk_lists(tfr_uknn* m, const int64_t* list_indptr /* [n+1] */, const int32_t* list_items, int64_t n, int32_t k,
                        const int64_t* excl_indptr /* [n+1] or NULL */, const int32_t* excl_items,
                        int32_t* items_out, float* scores_out);
int tfr_uknn_rank_items(tfr_uknn* m, const int32_t* users, int64_t n,
                        const int64_t* tgt_indptr /* [n+1] */, const int32_t* tgt_items,
                        const int64_t* excl_indptr /* [n+1] or NULL */, const int32_t* excl_items,
                        int32_t* ranks_out /* [tgt_indptr[n] - tgt_indptr[0]] */);
/* host-only, no device: what the launcher of the fit (which = 0: n_cols the users, k is K, n_rows the users), of the scoring
 * (which = 1: n_cols the items, k the query's k, n_rows the queries) or of the neighbour search of query lists (which = 2:
 * n_cols the users, k is K, n_rows the lists) will do - columns per slice, slices, rows per chunk, LDS bytes per workgroup
 * (the larger of that kernel and the merge), and how many list entries a wave takes at once (fit and search: entries of the
 * row whose bounds are fetched together; scoring: neighbour slots searched side by side).  Outputs may be NULL. */
int tfr_uknn_plan(int64_t n_cols, int32_t k, int64_t n_rows, int32_t which, int32_t* slice_width, int32_t* slices,
                  int64_t* row_chunk, int64_t* lds_bytes, int32_t* look_ahead);
const char* tfr_uknn_last_error(void);

/* ---- EASE (Steck 2019, "Embarrassingly Shallow Autoencoders"): a dense item x item model in closed form - DESIGN §32 ----------
 *      X: the binary user x item matrix, a CSR pattern [n_users, n_items] under the rules of tfr_knn_load (rows strictly
 *      increasing, no values).  n_i = the users of item i, c_ij = the users who have both i and j.
 *          G = X^T X + lambda I   float64: off the diagonal the exact integers c_ij, on it (double)n_i + lambda; lambda > 0, finite
 *          P = G^-1               float64, by a blocked Cholesky factorisation on the device; symmetric by construction: both
 *                                 triangles are stored with the same bits, and two solves of one G give the same bits
 *          B[i, j] = (float)(-P[i, j] / P[j, j]) for i != j: one correctly rounded float64 division, one rounding to float32;
 *          B[j, j] = +0.  B is a dense float32 [n_items, n_items], row-major.
 *          score(u, j) = the float32 add chain from +0, over i in N(u) ascending, of B[i, j]
 *      Every item is a candidate; a user with an empty list scores +0 everywhere and is served by id.  tfr_ease_topk /
 *      tfr_ease_topk_lists / tfr_ease_rank_items are tfr_topk / tfr_rank_items on these scores, word for word as their
 *      tfr_knn_* namesakes: 1 <= k <= 256, the key (the order-preserving uint32 of the score, then ~j), padding with item -1 /
 *      score -INFINITY, the exclusion CSR aligned with the queries with non-decreasing rows, target rows strictly increasing,
 *      duplicate users allowed, -1 for an excluded target, 0 <= rank < k exactly when top-K of k returns the target, at that
 *      position; a NaN score is never returned and never ranked.
 *      The dense matrices cost 12 bytes per entry: n_items > 32768 is refused with TFR_ERR_ARG before any device work.
 *      tfr_ease_load takes the user CSR and builds its transpose; a second load replaces the first and forgets the Gram matrix
 *      and the weights.  tfr_ease_gram builds G from the loaded pattern into the float64 buffer.  tfr_ease_set_gram takes a
 *      caller's full [n_items, n_items] matrix instead (weighted or time-decayed co-counts): it must be finite, bit-symmetric
 *      and have a positive diagonal (TFR_ERR_ARG otherwise); lambda is not added to it.  tfr_ease_solve inverts the float64
 *      buffer in place, forms B and frees the float64 buffer unless keep_inverse; elapsed_ms, if given, receives three device
 *      times: of the tfr_ease_gram that built the matrix (0 for a caller's), of the inverse and of the weights.  A pivot that
 *      is not positive and finite (the matrix is not positive definite) returns TFR_ERR_ARG, the message names the column;
 *      the model is then unfitted, holds no float64 matrix, and the handle stays usable.  tfr_ease_get_f64 copies rows
 *      [row_lo, row_lo + n_rows) of the float64 buffer out: G after gram / set_gram, P after a solve that kept it,
 *      TFR_ERR_STATE otherwise.  tfr_ease_get_weights / tfr_ease_set_weights read and write rows of B, so a fitted model moves
 *      without a refit: set_weights refuses values that are not finite (TFR_ERR_ARG); a handle without weights takes all
 *      rows in one call (TFR_ERR_STATE for fewer), which makes it fitted.  tfr_ease_topk queries resident users (their loaded
 *      rows are the lists); tfr_ease_topk_lists queries n given lists (a CSR from 0 with strictly increasing rows): it needs
 *      weights, not a load.
 *      Host pointers; every call synchronises.  Checked on the host before any device work (the model is left as it was):
 *      TFR_ERR_ARG for a lambda that is not positive and finite, k outside [1, 256], an indptr that does not start at 0 (user
 *      and list CSR) or decreases, a row out of order, rows outside the matrix; TFR_ERR_OOB for an id out of range;
 *      TFR_ERR_STATE for gram before a load, solve without a Gram matrix, get_weights, top-K and ranking without weights
 *      (top-K of users and ranking also before a load).  n = 0 and rows without targets are no-ops.  scores_out may be NULL. */
typedef struct tfr_ease tfr_ease;
int tfr_ease_create(tfr_ease** out, int64_t n_users, int64_t n_items, double lambda, int32_t device);
int tfr_ease_destroy(tfr_ease* m);
int tfr_ease_load(tfr_ease* m, const int64_t* indptr /* [n_users+1] */, const int32_t* items);
int tfr_ease_gram(tfr_ease* m);
int tfr_ease_set_gram(tfr_ease* m, const double* G /* [n_items,n_items] */);
int tfr_ease_solve(tfr_ease* m, int32_t keep_inverse, float* elapsed_ms /* [3]: Gram, inverse, weights; may be NULL */);
int tfr_ease_get_f64(tfr_ease* m, int64_t row_lo, int64_t n_rows, double* out /* [n_rows,n_items] */);
int tfr_ease_get_weights(tfr_ease* m, int64_t row_lo, int64_t n_rows, float* out /* [n_rows,n_items] */);
int tfr_ease_set_weights(tfr_ease* m, int64_t row_lo, int64_t n_rows, const float* in /* [n_rows,n_items] */);
int tfr_ease_topk(tfr_ease* m, const int32_t* users, int64_t n, int32_t k,
                  const int64_t* excl_indptr /* [n+1] or NULL */, const int32_t* excl_items,
                  int32_t* items_out /* [n,k] */, float* scores_out /* [n,k], may be NULL */);
int tfr_ease_topk_lists(tfr_ease* m, const int64_t* list_indptr /* [n+1] */, const int32_t* list_items, int64_t n, int32_t k,
                        const int64_t* excl_indptr /* [n+1] or NULL */, const int32_t* excl_items,
                        int32_t* items_out, float* scores_out);
int tfr_ease_rank_items(tfr_ease* m, const int32_t* users, int64_t n,
                        const int64_t* tgt_indptr /* [n+1] */, const int32_t* tgt_items,
                        const int64_t* excl_indptr /* [n+1] or NULL */, const int32_t* excl_items,
                        int32_t* ranks_out /* [tgt_indptr[n] - tgt_indptr[0]] */);
/* host-only, no handle and no device: what the launches to come will do.  For the fit - the factorisation block size, the
 * MFMA tile of the update kernel (tile x tile results per workgroup), and the float64 / float32 device bytes a fit allocates
 * (G / P with the work panel and the inverted diagonal blocks; B).  For which = 0 (the fit: k must be valid, n_rows is not
 * used) the slicing is the Gram kernel's and lds_bytes the largest of the fit's kernels; for which = 1 (scoring n_rows
 * queries for k) - columns per catalogue slice, slices, queries per chunk, LDS bytes per workgroup (the larger of the
 * scoring kernel and the merge) and how many list items a wave loads ahead.  TFR_ERR_ARG for what a launch would refuse:
 * n_items outside [1, 32768], k outside [1, 256], n_rows < 0.  Outputs may be NULL. */
int tfr_ease_plan(int64_t n_items, int32_t k, int64_t n_rows, int32_t which, int32_t* block, int32_t* tile, int64_t* lds_bytes,
                  int64_t* f64_bytes, int64_t* f32_bytes, int32_t* slice_width, int32_t* slices, int64_t* row_chunk,
                  int32_t* look_ahead);
const char* tfr_ease_last_error(void);

/* ---- PureSVD (Cremonesi, Koren, Turrin 2010): the rank-d truncated SVD of the interaction matrix (tfr_psvd_*) ----
 *      X is the binary user x item pattern (a CSR, rows strictly increasing), U x I.  With r = factors + oversample,
 *      1 <= factors, 0 <= oversample, r <= 128 (anything else: TFR_ERR_ARG at create, the message names r), in float64
 *      throughout:
 *          V <- orth(V0)                                  V0 [I, r] is the caller's start block (no device RNG)
 *          `iterations` times: W = X V, Z = X^T W, V <- orth(Z)
 *          W = X V, T = W^T W, (lambda, Qe) = eig(T)      eigenvalues descending, equal ones by column index; each
 *                                                         eigenvector's entry of largest magnitude (lowest index on a tie) > 0
 *          sigma_j = sqrt(max(lambda_j, 0)), item factors Q = V Qe[:, :factors], user factors P = X Q
 *      score(u, i) = p_u . q_i = (x_u V_d V_d^T)_i.  Every product with X is one kernel, out[row] = the sum of in[id] over
 *      the row's list in list order (lists past 256 entries: 256 at a time, the chunks' sums then added in chunk
 *      order), so P is bit for bit what tfr_psvd_fold_in gives for the list of a resident user.  orth is CholeskyQR
 *      twice: S = Z^T Z (the Gram of tfr_ials_gram, same slice order), R = chol(S) upper, V = Z R^-1.  A pivot that is not
 *      finite or not above 2^-44 times its column's entry of S (the block has fewer independent columns than r: r > rank X)
 *      ends the call with TFR_ERR_ARG; the message names the orthonormalisation (0 = the start block's), the pass (1, 2) and
 *      the column, nothing further runs, and the handle is loaded, not fitted: an earlier fit is forgotten.  eig is a cyclic Jacobi iteration in
 *      one workgroup, round-robin pairs in a fixed order, rotating where |t_pq| > 2^-52 max|T|, until a sweep makes no
 *      rotation; a rotation in sweep 30 is TFR_ERR_ARG.  tfr_psvd_sweeps: sweeps of the last eigen step, the clean one included.
 *      All results are the same bits from run to run.
 *
 *      tfr_psvd_load: the user CSR (checked on the host first: a refused load leaves the model as it was); a load forgets
 *      the factors.  tfr_psvd_fit: ms [3] (may be NULL) = device time of the products, of the orthonormalisations, of the
 *      eigen step with the last products.  tfr_psvd_get: what = 0 sigma [factors], 1 Q [I, factors], 2 P [U, factors],
 *      3 all r Ritz values lambda (TFR_ERR_STATE after set_factors).  tfr_psvd_set_factors: Q and sigma from a fitted model;
 *      needs a load; P = X Q is recomputed.  tfr_psvd_residuals: out[j] = ||X^T (X q_j) - sigma_j^2 q_j||_2 / sigma_0^2 from
 *      the factors as they stand (two products).  The stages alone: tfr_psvd_multiply (side 0: out [U, cols] = X in,
 *      side 1: out [I, cols] = X^T in; 1 <= cols <= 128), tfr_psvd_orthonormalise (block [n, cols] in place; S_out, R_out
 *      [2, cols, cols] of the two passes, may be NULL; needs no load), tfr_psvd_eig (T symmetric bit for bit; lambda_out [r],
 *      Q_out [r, r] eigenvectors in columns; needs no load).  tfr_psvd_fold_in: p = x Q for n lists the model does not
 *      hold (a CSR from 0, rows strictly increasing; an empty list gives zeros); out [n, factors] may be NULL: the rows stay
 *      on the device for tfr_psvd_export_f32, which writes rows of Q (which = 0), P (1) or the last fold-in (2) as float32
 *      into a device pointer of the caller.  TFR_ERR_STATE: fit, multiply, set_factors, residuals before a load; get,
 *      residuals, fold_in, export_f32 before factors.  TFR_ERR_OOB: an id out of range. */
typedef struct tfr_psvd tfr_psvd;
int tfr_psvd_create(tfr_psvd** out, int64_t n_users, int64_t n_items, int32_t factors, int32_t oversample, int32_t device);
int tfr_psvd_destroy(tfr_psvd* m);
int tfr_psvd_load(tfr_psvd* m, const int64_t* indptr /* [n_users+1] */, const int32_t* items);
int tfr_psvd_fit(tfr_psvd* m, const double* V0 /* [n_items,r] */, int32_t iterations, float* ms /* [3]; may be NULL */);
int tfr_psvd_get(tfr_psvd* m, int32_t what, double* out);
int tfr_psvd_sweeps(tfr_psvd* m, int32_t* out);
int tfr_psvd_set_factors(tfr_psvd* m, const double* Q /* [n_items,factors] */, const double* sigma /* [factors] */);
int tfr_psvd_residuals(tfr_psvd* m, double* out /* [factors] */);
int tfr_psvd_multiply(tfr_psvd* m, int32_t side, const double* in, int32_t cols, double* out);
/* the product kernel alone on a zeroed device block, `reps` times: ms_out [reps] device times (events); needs a load */
int tfr_psvd_product_ms(tfr_psvd* m, int32_t side, int32_t cols, int32_t reps, float* ms_out);
int tfr_psvd_orthonormalise(tfr_psvd* m, int64_t n, double* block /* [n,cols] */, int32_t cols, double* S_out, double* R_out);
int tfr_psvd_eig(tfr_psvd* m, const double* T /* [r,r] */, int32_t r, double* lambda_out, double* Q_out);
int tfr_psvd_fold_in(tfr_psvd* m, int64_t n, const int64_t* indptr /* [n+1] */, const int32_t* ids, double* out /* [n,factors] or NULL */);
int tfr_psvd_export_f32(tfr_psvd* m, int32_t which, int64_t row_lo, int64_t n_rows, void* dst_devptr);
/* The launch shapes, computed on the host (no device): r, the lanes of a wave that own columns (64 at every width: a wave
 * per row, two columns per lane, the lanes past r / 2 masked), the chunk of a long list, the entries a wave loads ahead, the
 * sweep cap, the largest LDS of the fit's launches, the float64 device bytes of a fit, and the slices of r * r doubles its
 * Gram partial buffer holds: the larger of ceil(n / rows(n)) over the two sides, rows(n) the ALS Gram's slice rule, which is
 * not monotonic in n.  Each out may be NULL.  TFR_ERR_ARG for what create refuses. */
int tfr_psvd_plan(int64_t n_users, int64_t n_items, int32_t factors, int32_t oversample, int32_t* r, int32_t* lanes, int32_t* chunk,
                  int32_t* ahead, int32_t* sweep_cap, int64_t* lds_bytes, int64_t* device_bytes, int64_t* gram_slices);
const char* tfr_psvd_last_error(void);

/* ---- SLIM (Ning & Karypis 2011, "Sparse Linear Methods for Top-N Recommender Systems"): elastic-net item weights - DESIGN §34 --
 *      X as for EASE.  A = X^T X + beta I in float64: exactly tfr_ease_gram's matrix with lambda = beta (beta >= 0, finite).
 *      For each item j the column w of W minimises
 *          1/2 w^T A w - a_j^T w + l1 * sum|w|,   w[j] = 0,   w >= 0 when positive
 *      where a_j is column j of A (its entry j is never read).  In sklearn's ElasticNet(alpha, l1_ratio) terms over the U
 *      users: l1 = U * alpha * l1_ratio, beta = U * alpha * (1 - l1_ratio).  The solver is cyclic coordinate descent on the
 *      residual q[i] = a_j[i] - sum over k != i of A[i, k] w[k]; the device produces the bits of
 *          q = a_j;  w = 0;  d[i] = A[i, i]
 *          for sweep in 1..max_iter:
 *              dmax = 0
 *              for i in 0..n-1 ascending, i != j, d[i] > 0:           (d[i] <= 0: w[i] stays 0)
 *                  positive:      t = q[i] - l1;   wn = t > 0 ? t / d[i] : 0
 *                  not positive:  t = |q[i]| - l1; wn = t > 0 ? copysign(t / d[i], q[i]) : 0
 *                  dl = wn - w[i]
 *                  if dl != 0:
 *                      for k != i:  q[k] = q[k] - (dl * A[i, k])      (the product rounded, then the difference: no fma)
 *                      w[i] = wn;  updates += 1;  dmax = max(dmax, |dl|)
 *              if dmax <= tol * max|w|:  converged; stop              (both 0 stop too)
 *          W[i, j] = (float)w[i] where w[i] != 0, +0 elsewhere
 *      in float64 throughout, whatever the launch geometry: two solves give the same bits.  W is a dense float32
 *      [n_items, n_items], row-major, and scores, top-K and ranks are EASE's on it, word for word (tfr_ease_topk and its
 *      neighbours above): score(u, j) = the float32 add chain from +0, over i in N(u) ascending, of W[i, j].
 *      A column's residual lives in the LDS of one workgroup: n_items > 16384 is refused with TFR_ERR_ARG before any device work.
 *      tfr_slim_load takes the user CSR; a second load replaces the first and forgets the Gram matrix, the weights and the
 *      statistics.  tfr_slim_gram builds A from the loaded pattern.  tfr_slim_set_gram takes a caller's full matrix instead: it
 *      must be finite and bit-symmetric (TFR_ERR_ARG otherwise); beta is not added to it.  tfr_slim_get_gram copies rows of A
 *      out.  tfr_slim_solve runs the solver for every column and keeps A, so another solve (another l1) needs no new Gram
 *      matrix; elapsed_ms, if given, receives two device times: of the tfr_slim_gram that built A (0 for a caller's) and of
 *      the solve.  A column whose weights leave the finite range (a caller's matrix with a tiny diagonal) returns TFR_ERR_ARG
 *      naming it, and the model is unfitted.  tfr_slim_get_stats copies out, per column of the last solve, the sweeps run, the
 *      coordinate updates applied and whether the stopping rule was met (each may be NULL); TFR_ERR_STATE when the weights
 *      are not a solve's.  tfr_slim_get_weights / tfr_slim_set_weights follow tfr_ease_get_weights / tfr_ease_set_weights.
 *      Host pointers; every call synchronises.  Checked on the host before any device work (the model is left as it was):
 *      TFR_ERR_ARG for a beta, l1 or tol that is negative or not finite, max_iter < 1, k outside [1, 256] and the CSR errors of
 *      tfr_ease_*; TFR_ERR_OOB for an id out of range; TFR_ERR_STATE for gram before a load, solve and get_gram without a Gram
 *      matrix, get_weights, top-K and ranking without weights (top-K of users and ranking also before a load). */
typedef struct tfr_slim tfr_slim;
int tfr_slim_create(tfr_slim** out, int64_t n_users, int64_t n_items, double beta, int32_t device);
int tfr_slim_destroy(tfr_slim* m);
int tfr_slim_load(tfr_slim* m, const int64_t* indptr /* [n_users+1] */, const int32_t* items);
int tfr_slim_gram(tfr_slim* m);
int tfr_slim_set_gram(tfr_slim* m, const double* A /* [n_items,n_items] */);
int tfr_slim_get_gram(tfr_slim* m, int64_t row_lo, int64_t n_rows, double* out /* [n_rows,n_items] */);
int tfr_slim_solve(tfr_slim* m, double l1, int32_t positive, int32_t max_iter, double tol,
                   float* elapsed_ms /* [2]: Gram, solve; may be NULL */);
int tfr_slim_get_stats(tfr_slim* m, int32_t* sweeps /* [n_items] */, int32_t* updates /* [n_items] */, int32_t* converged /* [n_items] */);
int tfr_slim_get_weights(tfr_slim* m, int64_t row_lo, int64_t n_rows, float* out /* [n_rows,n_items] */);
int tfr_slim_set_weights(tfr_slim* m, int64_t row_lo, int64_t n_rows, const float* in /* [n_rows,n_items] */);
int tfr_slim_topk(tfr_slim* m, const int32_t* users, int64_t n, int32_t k,
                  const int64_t* excl_indptr /* [n+1] or NULL */, const int32_t* excl_items,
                  int32_t* items_out /* [n,k] */, float* scores_out /* [n,k], may be NULL */);
int tfr_slim_topk_lists(tfr_slim* m, const int64_t* list_indptr /* [n+1] */, const int32_t* list_items, int64_t n, int32_t k,
                        const int64_t* excl_indptr /* [n+1] or NULL */, const int32_t* excl_items,
                        int32_t* items_out, float* scores_out);
int tfr_slim_rank_items(tfr_slim* m, const int32_t* users, int64_t n,
                        const int64_t* tgt_indptr /* [n+1] */, const int32_t* tgt_items,
                        const int64_t* excl_indptr /* [n+1] or NULL */, const int32_t* excl_items,
                        int32_t* ranks_out /* [tgt_indptr[n] - tgt_indptr[0]] */);
/* host-only, no handle and no device.  For which = 0 (the fit: k must be valid, n_rows is not used): the window (coordinates
 * the solver examines at once = threads per workgroup), the solver's grid, the LDS bytes of one solver workgroup (the Gram
 * kernel's are tfr_ease_plan's), whether the column's weights live in LDS beside q (0: in a global scratch row per workgroup),
 * and the float64 / float32 device bytes of a fit (A, its diagonal and the scratch rows; W).  For which = 1 (scoring n_rows
 * queries for k): tfr_ease_plan's scoring slicing.  TFR_ERR_ARG for n_items outside [1, 16384], k outside [1, 256],
 * n_rows < 0.  Outputs may be NULL. */
int tfr_slim_plan(int64_t n_items, int32_t k, int64_t n_rows, int32_t which, int32_t* window, int32_t* grid, int64_t* lds_bytes,
                  int32_t* w_in_lds, int64_t* f64_bytes, int64_t* f32_bytes, int32_t* slice_width, int32_t* slices,
                  int64_t* row_chunk, int32_t* look_ahead);
const char* tfr_slim_last_error(void);

/* ---- batched per-user fine-tuning: every user of adaptive_test.py:87-116 / non_adaptive_test.py:56-87 in one launch -----------
 *      A schedule: for user u = users[x] (each at most once), training rows items / rates [row_ptr[x], row_ptr[x+1]) and rounds
 *      [round_ptr[x], round_ptr[x+1]).  Round k first predicts ask_items[k] with the parameters of the moment (its logit, the
 *      forward's ((dot + mu) + bu) + bi, goes to ask_logits_out[k]), then runs nsteps training steps on the first prefix_len[k]
 *      rows of its user (1 <= prefix_len[k] <= the user's rows): what tfr_forward + tfr_train_steps_repeat do per round.
 *      round_seq[k] = the step, counted from this call's start, at which the sequential drivers would start round k (NULL =
 *      k * nsteps, user-major order); with Adam each step uses the beta powers of that sequential position (the model's float32
 *      recurrence replayed on the host), so lr_t is the sequential one.  Outputs: round_loss_out[k] = data loss of round k's
 *      last step; final_logits_out[row] = pre-update logits of each user's last step over its last round's prefix (other rows
 *      untouched).  Both may be NULL.
 *      Needs bias_global, item_bias and item_features frozen and SGD or lazy Adam (TFR_ERR_ARG otherwise: tf1 Adam couples the
 *      users).  Ids are checked on the host (TFR_ERR_OOB), the schedule's shape too (TFR_ERR_ARG), before any device work; on an
 *      error nothing changes.  On success the users' user_features / user_bias rows and their slots are written back, the step
 *      counter advances by n_rounds * nsteps and the beta powers end where the sequential drivers leave them; every other row
 *      and table is untouched.  No atomics and fixed summation orders: a user's results are bit-identical whichever users share
 *      the call.  Runs on the model's stream and synchronises.  Matches the sequential path to float32 rounding (the sums run in
 *      a different order), not bit for bit. */
int tfr_finetune_users(tfr_model* m, int64_t n_users, const int32_t* users, const int64_t* row_ptr /* [n_users+1] */,
                       const int32_t* items, const float* rates, const int64_t* round_ptr /* [n_users+1] */,
                       const int32_t* ask_items, const int32_t* prefix_len, const int64_t* round_seq /* or NULL */,
                       int32_t nsteps, float* ask_logits_out /* [n_rounds] */, float* round_loss_out /* [n_rounds] or NULL */,
                       float* final_logits_out /* [n_rows] or NULL */);
/* host-only, no device: what the launcher does for a call whose largest user has max_rows rows - LDS bytes per workgroup (a CU
 * has 160 KiB), users whose rows are staged in LDS (at most this many rows; larger users read their item rows from global
 * memory), waves (users) per workgroup */
int tfr_finetune_plan(int32_t dim, int64_t max_rows, int64_t* lds_bytes, int32_t* rows_staged, int32_t* waves_per_block);

/* ---- SVD++ (Koren, "Factorization Meets the Neighborhood", KDD 2008): the third model of the reference README - DESIGN §14 ----
 *      A tfr_svdpp wraps a tfr_model (its five tables, optimiser, hyper-parameters, step and stream) and adds Y [I, D], the
 *      implicit item factors, with their Adam slots, and the implicit sets N(u): a CSR [U, I] given by the caller.
 *          s_u = 1/sqrt(|N(u)|), z_u = s_u * sum_{j in N(u)} Y[j] (z_u = 0 for an empty row),  e = P[u] + z_u
 *          logit = ((dot(e, Q'[i]) + mu) + bu[u]) + bi[i]          (Q' = |Q| under item_abs; the SVD forward's add order)
 *      Loss and heads are the SVD model's; the regulariser adds, per batch entry, 1/2 sum_{j in N(u)} ||Y[j]||^2.  Gradients
 *      per occurrence with g = d loss / d logit: dP = g Q' + lam P, dQ = g e (x sign(Q) under item_abs) + lam Q, biases and mu
 *      as in SVD, and dY[j] += g s_u Q'[i] + lam Y[j] for every j in N(u).  SGD or lazy Adam (touched rows); tf1 Adam is
 *      refused (TFR_ERR_STATE).  Every quantity uses the tables before the step.  Sums have a fixed order: bit-identical
 *      run to run.  Table ids: TFR_MU..TFR_Q and TFR_Y, each + TFR_SLOT_M / TFR_SLOT_V; frozen bit TFR_Y freezes Y.
 *      Ids of a batch out of range void the step (every table) and the next synchronising call returns TFR_ERR_OOB, as the
 *      SVD step.  Training, forward, top-K and ranking before tfr_svdpp_set_implicit return TFR_ERR_STATE. */
typedef struct tfr_svdpp tfr_svdpp;
enum { TFR_Y = 5 };
int tfr_svdpp_create(tfr_svdpp** out, int64_t user_num, int64_t item_num, int32_t dim, const tfr_opts* opts);
int tfr_svdpp_destroy(tfr_svdpp* m);
int tfr_svdpp_set_table(tfr_svdpp* m, int32_t which, const float* host, int64_t n);
int tfr_svdpp_get_table(tfr_svdpp* m, int32_t which, float* host, int64_t n);
/* tfr_init_tables of the wrapped model plus Y ~ truncated normal(feature_stddev); zeroes Y's slots */
int tfr_svdpp_init(tfr_svdpp* m, uint64_t seed, float feature_stddev, float bias_stddev);
/* N(u): indptr [user_num + 1] from 0, non-decreasing; items with every row strictly increasing.  Checked on the host before
 * any device work: an item outside [0, item_num) gives TFR_ERR_OOB, anything else malformed TFR_ERR_ARG.  Resident (with its
 * transpose) until replaced; synchronises. */
int tfr_svdpp_set_implicit(tfr_svdpp* m, const int64_t* indptr, const int32_t* items);
int tfr_svdpp_set_frozen(tfr_svdpp* m, uint32_t mask);
int tfr_svdpp_set_hyper(tfr_svdpp* m, float lr, float reg);
int tfr_svdpp_get_step(tfr_svdpp* m, int64_t* step, float* beta1_power, float* beta2_power);
int tfr_svdpp_set_step(tfr_svdpp* m, int64_t step, float beta1_power, float beta2_power);
int tfr_svdpp_forward(tfr_svdpp* m, const int32_t* user, const int32_t* item, int64_t batch, float* logits_out);
int tfr_svdpp_forward_dev(tfr_svdpp* m, const int32_t* d_user, const int32_t* d_item, int64_t batch, float* d_logits);
/* sum_k (infer_k - rate_k)^2 and the count of infer == rate, as tfr_eval */
int tfr_svdpp_eval(tfr_svdpp* m, const int32_t* user, const int32_t* item, const float* rate, int64_t batch,
                   double* sum_sq_err_out, int64_t* n_equal_out);
/* one minibatch: pre-update logits (may be NULL), data loss and regulariser, as tfr_train_step */
int tfr_svdpp_train_step(tfr_svdpp* m, const int32_t* user, const int32_t* item, const float* rate, int64_t batch,
                         float* logits_out, float* loss_out, float* reg_out);
int tfr_svdpp_train_step_dev(tfr_svdpp* m, const int32_t* d_user, const int32_t* d_item, const float* d_rate, int64_t batch,
                             float* d_logits /* may be NULL */);
/* tfr_topk / tfr_topk_dev / tfr_rank_items with e = P[u] + z_u in place of P[u]: the same keys, so rank < K exactly when
 * tfr_svdpp_topk(K) returns the item, at that position */
int tfr_svdpp_topk(tfr_svdpp* m, const int32_t* users, int64_t n_users, int32_t k, const int64_t* excl_indptr,
                   const int32_t* excl_items, int32_t* items_out, float* scores_out);
int tfr_svdpp_topk_dev(tfr_svdpp* m, const int32_t* d_users, int64_t n_users, int32_t k, const int64_t* d_excl_indptr,
                       const int32_t* d_excl_items, int32_t* d_items_out, float* d_scores_out);
int tfr_svdpp_rank_items(tfr_svdpp* m, const int32_t* users, int64_t n_users, const int64_t* tgt_indptr,
                         const int32_t* tgt_items, const int64_t* excl_indptr, const int32_t* excl_items, int32_t* ranks_out);
int tfr_svdpp_get_stream(tfr_svdpp* m, void** hip_stream);
int tfr_svdpp_sync(tfr_svdpp* m);            /* drains the stream; reports deferred TFR_ERR_OOB */
const char* tfr_svdpp_last_error(void);

/* ---- BPR (Rendle et al., "BPR: Bayesian Personalized Ranking from Implicit Feedback", UAI 2009) - DESIGN §15 ----------
 *      A BPR step trains the SVD model's own tables (tables, optimiser, hyper-parameters, step counter and stream of the
 *      tfr_model) on triples (u, i, j): i a positive of u, j a negative.  For a triple, with Q' = |Q| under item_abs,
 *          s(u, k) = dot(P[u], Q'[k]) + bi[k]      dot: per-lane f32 fmaf chains over f = lane + 64 t, then a butterfly sum
 *          x = s(u, i) - s(u, j)                   (mu and bu cancel: a BPR step never reads or writes them)
 *          data = sum_b softplus(-x_b)             (max(-x, 0) + log1p(exp(-|x|)))
 *          reg  = 1/2 sum_b (||P[u_b]||^2 + ||Q[i_b]||^2 + ||Q[j_b]||^2)  (+ 1/2 (bi[i_b]^2 + bi[j_b]^2) with reg_bias)
 *          cost = data + lam reg                   (loss_out = data, reg_out = reg, as tfr_train_step)
 *      Per triple, g = -sigmoid(-x): dP[u] = g (Q'[i] - Q'[j]) + lam P[u]; dQ[i] = g P[u] (x sign Q[i] under item_abs)
 *      + lam Q[i]; dQ[j] = -g P[u] (x sign Q[j]) + lam Q[j]; dbi[i] = g, dbi[j] = -g (each + lam bi with reg_bias).  An
 *      item that is the positive of one triple and the negative of another sums both roles.  Every quantity uses the tables
 *      as they were before the step.  SGD or lazy Adam on the touched rows (the SVD step's sparse Adam); tf1 Adam gives
 *      TFR_ERR_STATE.  Frozen bits TFR_BI, TFR_P, TFR_Q are honoured.  The step counter and the beta powers advance once
 *      per step.  The model's loss option does not apply.  Sums run in a fixed order: bit-identical run to run, and a
 *      user's rows get the same bits whichever other users (touching none of its rows) share the batch.  An id out of range
 *      voids the step (every table) and the next synchronising call returns TFR_ERR_OOB, as the SVD step.
 *
 *      Negative sampler, counter-based (all arithmetic mod 2^64):
 *          mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
 *          k   = mix(mix(seed ^ 0x9E3779B97F4A7C15) ^ step)     step = the model's step counter before this step
 *          r_a = mix(k ^ ((b << 6) | a))                      b = position in the batch, a = attempt, 0 <= a < attempts <= 64
 *          j_a = ((r_a >> 32) * item_num) >> 32
 *      j = the first j_a not in row u of the positives.  If every attempt lands on a positive the triple is skipped: it is
 *      absent from the batch (no data, no regulariser, no gradient, no lazy-Adam touch) and its negative reads -1.
 *      Defaults: seed 0, attempts 16.  Negatives given by the caller are used as given: checked as ids, never rejected,
 *      j == i legal.
 *
 *      Positives: a CSR [user_num, item_num], indptr from 0, non-decreasing, each row strictly increasing; checked on the
 *      host before any device work (TFR_ERR_OOB for an item out of range, TFR_ERR_ARG otherwise); resident until replaced;
 *      the call synchronises.  Sampling and training calls before it return TFR_ERR_STATE. */
int tfr_bpr_set_positives(tfr_model* m, const int64_t* indptr /* [user_num + 1] */, const int32_t* items);
/* seed and attempts (1..64) of the sampler; kept until changed */
int tfr_bpr_set_sampler(tfr_model* m, uint64_t seed, int32_t attempts);
/* the sampler alone, at counter `step`, for host users (checked on the host: TFR_ERR_OOB); synchronises */
int tfr_bpr_negatives(tfr_model* m, const int32_t* user, int64_t batch, int64_t step, int32_t* neg_out);
/* one BPR step on host columns; neg NULL = sample.  neg_out [batch] receives the negatives used (-1 = skipped),
 * n_skipped_out the number of skipped triples.  Any output may be NULL; synchronises. */
int tfr_bpr_train_step(tfr_model* m, const int32_t* user, const int32_t* pos, const int32_t* neg /* NULL = sample */,
                       int64_t batch, int32_t* neg_out, float* loss_out, float* reg_out, int64_t* n_skipped_out);
/* the same on device columns, asynchronous (id errors surface at the next synchronising call) */
int tfr_bpr_train_step_dev(tfr_model* m, const int32_t* d_user, const int32_t* d_pos, const int32_t* d_neg /* NULL = sample */,
                           int64_t batch, int32_t* d_neg_out /* may be NULL */);
/* nsteps x { e = np.random.randint(0, nnz, batch) from the model's MT19937 stream (as tfr_train_steps_drawn draws);
 * (u, i) = entry e of the positives CSR; one BPR step with sampled negatives }, all on the device.  Cancels the SVD
 * path's run-ahead draw first and draws into its own buffer.  loss_out[nsteps] (may be NULL; then the call does not
 * synchronise): data term per step. */
int tfr_bpr_train_steps_drawn(tfr_model* m, int64_t batch, int32_t nsteps, float* loss_out);

/* ---- WARP (Weston, Bengio, Usunier, "WSABIE: Scaling Up To Large Vocabulary Image Annotation", IJCAI 2011) - DESIGN §30 --
 *      A WARP step trains the SVD model's own tables as a BPR step does, through a trainer handle created from the model and
 *      bound to it.  The positives and the sampler's seed and attempts are the model's (tfr_bpr_set_positives,
 *      tfr_bpr_set_sampler); the trainer holds the margin.  A trainer must not outlive its model: tfr_destroy on a model
 *      with a live trainer returns TFR_ERR_STATE and leaves both intact.
 *
 *      Scores and candidates.  For a triple (u, i), s(u, k), Q' and the dot's operation order are BPR's.  With
 *          key = mix(mix(seed ^ 0x9E3779B97F4A7C15) ^ step)        step = the model's step counter before this step
 *          c_t = ((mix(key ^ ((b << 6) | t)) >> 32) * item_num) >> 32      for t = 0 .. attempts - 1
 *      the candidates are the draws tfr_bpr_negatives makes at the same seed, step and position b.
 *
 *      Violator search.  The candidates are walked in order, n from 0.  A candidate in row u of the positives is passed
 *      over and not counted.  Otherwise n += 1 and
 *          x_t = (d_i + bi[i]) - (d_c + bi[c])     f32, d_k = dot(P[u], Q'[k]) as in a BPR step, this order of operations
 *      and if x_t < margin the negative is j = c_t, the trial count N = n, and the search stops.  If no candidate violates,
 *      the triple is skipped: neg = -1, N = 0; it contributes nothing and touches nothing, exactly as a skipped BPR triple.
 *      Every score uses the tables as they were before the step.  The x the step then uses for (u, i, j) is formed by the
 *      same function on the same operands: it has the bits the search compared, so margin - x > 0 for every live triple
 *      of a search.
 *
 *      Weight.  w = logf((float)max(1, (item_num - 1) / N)), the division in integers.  item_num >= 2 is required: every
 *      searching or training call on a model with one item returns TFR_ERR_ARG.
 *
 *      Step.
 *          data = sum_b w_b max(0, margin - x_b)
 *          reg and cost = data + lam reg as in a BPR step
 *      Per live triple g_b = -w_b if x_b < margin, else 0; dP, dQ[i], dQ[j], dbi[i], dbi[j] are BPR's formulas with that g.  A
 *      live triple with g = 0 (a caller's negative that does not violate) still gets its lam terms and its lazy-Adam touch.
 *      As in a BPR step: SGD or lazy Adam on the touched rows, tf1 Adam refused with TFR_ERR_STATE, the frozen bits TFR_BI,
 *      TFR_P, TFR_Q, one advance of the step counter and the beta powers per step, an id out of range voids the step (every
 *      table), mu and bu are never read or written, every sum runs in a fixed order.
 *
 *      Negatives given by the caller are used as given (checked as ids, never rejected, j == i legal) with N = 1 for every
 *      triple, so w = logf(item_num - 1).
 *
 *      Consequences: with margin = +INFINITY the negatives equal tfr_bpr_negatives' and every N is 1; with margin =
 *      -INFINITY every triple is skipped.  A NaN margin is TFR_ERR_ARG.
 *
 *      Calls before tfr_bpr_set_positives return TFR_ERR_STATE.  Errors and the rollback of a void step follow
 *      tfr_bpr_train_step. */
typedef struct tfr_warp tfr_warp;
/* the trainer of model m with this margin; any number may be bound to one model */
int tfr_warp_create(tfr_warp** out, tfr_model* m, float margin);
int tfr_warp_destroy(tfr_warp* w);           /* NULL is a no-op; drains the model's stream */
int tfr_warp_set_margin(tfr_warp* w, float margin);
/* the search alone on the current tables, at counter `step`, for host users and positives (checked on the host:
 * TFR_ERR_OOB); neg_out [batch] (-1 = no violator), trials_out [batch] (may be NULL) the trial counts N; synchronises */
int tfr_warp_negatives(tfr_warp* w, const int32_t* user, const int32_t* pos, int64_t batch, int64_t step, int32_t* neg_out,
                       int32_t* trials_out);
/* one WARP step on host columns; neg NULL = search.  neg_out [batch] receives the negatives used (-1 = skipped), trials_out
 * [batch] the trial counts, n_skipped_out the number of skipped triples.  Any output may be NULL; synchronises. */
int tfr_warp_train_step(tfr_warp* w, const int32_t* user, const int32_t* pos, const int32_t* neg /* NULL = search */,
                        int64_t batch, int32_t* neg_out, int32_t* trials_out, float* loss_out, float* reg_out,
                        int64_t* n_skipped_out);
/* the same on device columns, asynchronous (id errors surface at the next synchronising call of the model) */
int tfr_warp_train_step_dev(tfr_warp* w, const int32_t* d_user, const int32_t* d_pos, const int32_t* d_neg /* NULL = search */,
                            int64_t batch, int32_t* d_neg_out /* may be NULL */, int32_t* d_trials_out /* may be NULL */);
/* tfr_bpr_train_steps_drawn with WARP steps: it consumes the model's MT19937 stream exactly as that call does (from one
 * generator state both draw the same pairs).  loss_out[nsteps] (may be NULL; then the call does not synchronise). */
int tfr_warp_train_steps_drawn(tfr_warp* w, int64_t batch, int32_t nsteps, float* loss_out);

/* ---- nearest neighbours in factor space: "what is like item i", "who is like user u" - DESIGN §17 -----------------------
 *      One table T [R, dim] gives the query rows and the candidate rows: TFR_NB_ITEMS = item_features (|Q| with item_abs),
 *      TFR_NB_USERS = user_features; for SVD++ users the effective rows P[u] + z_u that tfr_svdpp_topk scores with; for the
 *      FM the feature rows V.
 *          dot(a, b)    = the f32 fmaf chain over f = 0..dim-1 ascending, from +0, of T[a,f] * T[b,f] (the tfr_topk chain,
 *                         no bias terms)
 *          ss[r]        = the f32 fmaf chain over f ascending, from +0, of T[r,f]^2;  rn[r] = 1 / sqrtf(ss[r]), 0 if ss[r] == 0
 *          TFR_NB_DOT:    s(a, b) = dot(a, b)
 *          TFR_NB_COSINE: s(a, b) = (dot(a, b) * rn[a]) * rn[b], both products f32, in that order; every score of a zero row
 *                         is +0, so it is orderable and not NaN
 *      Per query row a = rows[r] the k best candidates b in [lo, hi) (0 <= lo < hi <= R; ids are row ids of T whatever the
 *      range) by s descending, then b ascending - the tfr_topk key.  Never returned: a itself, the rows of the query's
 *      exclusion row, candidates whose score is NaN.  Slots past the eligible candidates hold id -1 / score -INFINITY.
 *      1 <= k <= 256; duplicate queries allowed; n = 0 is a no-op.
 *      Exclusions: optional CSR (excl_indptr [n+1], excl) aligned with `rows`, each row non-decreasing row ids of T.  The host
 *      entries check ids and order first (TFR_ERR_OOB for a query or excluded id out of range, TFR_ERR_ARG for an unsorted
 *      row, a bad k, metric, table or range; outputs untouched); tfr_neighbours_dev checks on the device with the error bits
 *      of tfr_topk_dev and reports through the next synchronising call.  Reads the tables only; runs on the model's stream;
 *      the host entries synchronise, tfr_neighbours_dev does not.  scores_out may be NULL.
 *      The inverse norms live on the device and are rebuilt when the table may have changed since they were made: after any
 *      training step (the step counter moved) and after tfr_set_table, tfr_init_tables, tfr_set_step, tfr_set_frozen or a
 *      voided step; once tfr_table_devptr has handed a table out for writing they are rebuilt on every cosine query. */
enum { TFR_NB_ITEMS = 0, TFR_NB_USERS = 1 };
enum { TFR_NB_DOT = 0, TFR_NB_COSINE = 1 };
int tfr_neighbours(tfr_model* m, int32_t which, int32_t metric, const int32_t* rows, int64_t n, int32_t k,
                   const int64_t* excl_indptr /* [n+1] or NULL */, const int32_t* excl, int64_t lo, int64_t hi,
                   int32_t* ids_out /* [n,k] */, float* scores_out /* [n,k], may be NULL */);
int tfr_neighbours_dev(tfr_model* m, int32_t which, int32_t metric, const int32_t* d_rows, int64_t n, int32_t k,
                       const int64_t* d_excl_indptr, const int32_t* d_excl, int64_t lo, int64_t hi,
                       int32_t* d_ids_out, float* d_scores_out);
/* SVD++: items as tfr_neighbours; users on e_u = P[u] + z_u, rebuilt for every user by each call (needs the implicit sets).
 * Host pointers; synchronises. */
int tfr_svdpp_neighbours(tfr_svdpp* m, int32_t which, int32_t metric, const int32_t* rows, int64_t n, int32_t k,
                         const int64_t* excl_indptr, const int32_t* excl, int64_t lo, int64_t hi,
                         int32_t* ids_out, float* scores_out);
int tfr_svdpp_neighbours_dev(tfr_svdpp* m, int32_t which, int32_t metric, const int32_t* d_rows, int64_t n, int32_t k,
                             const int64_t* d_excl_indptr, const int32_t* d_excl, int64_t lo, int64_t hi,
                             int32_t* d_ids_out, float* d_scores_out);
/* FM: features against the features [lo, hi) of V - a block of the design matrix, for example the item block */
int tfr_fm_neighbours(tfr_fm* m, int32_t metric, const int32_t* features, int64_t n, int32_t k,
                      const int64_t* excl_indptr, const int32_t* excl, int64_t lo, int64_t hi,
                      int32_t* ids_out, float* scores_out);
/* host-only, no device: what the launcher will do for n query rows against n_candidates rows - LDS bytes per workgroup
 * (the larger of the scoring and the merge kernel; k_row_rnorm uses none), query rows per scoring workgroup, candidate
 * slices, query rows per chunk */
int tfr_neighbours_plan(int32_t dim, int32_t k, int64_t n, int64_t n_candidates,
                        int64_t* lds_bytes, int32_t* rows_per_block, int32_t* slices, int64_t* row_chunk);

/* ---- per-kernel timing with HIP events on the model's stream (bench.py roofline) -------- */
enum {
    TFR_K_FORWARD = 0,        /* gather-dot forward (+ fused loss/grad when training)       */
    TFR_K_SORT = 1,           /* key sorts of both id columns                               */
    TFR_K_REDUCE_ITEM = 2,    /* deterministic segmented reduce, item side                  */
    TFR_K_REDUCE_USER = 3,    /* deterministic segmented reduce (+ fused lazy Adam), user   */
    TFR_K_APPLY = 4,          /* Adam / SGD apply kernels                                   */
    TFR_K_FINALIZE = 5,       /* scalar reduction + bias_global update                      */
    TFR_K_GATHER = 6,         /* resident-store triple gather                               */
    TFR_K_DRAW = 7,           /* MT19937 id draw (timed on its own side stream)             */
    TFR_K_COUNT = 8
};
int tfr_profile(tfr_model* m, int32_t enable);                 /* enable resets the counters */
/* "slot=kernel<template args>;..." - the kernels one training step of this model launches at this batch
 * size, spelled as rocprofv3 prints them (what the slots above time) */
int tfr_kernel_plan(tfr_model* m, int64_t batch, char* buf, int64_t buflen);
int tfr_profile_read(tfr_model* m, int32_t kernel, double* total_ms, int64_t* launches);
/* "k_forward<G, VEC, MODE, 4, PNT>;grid=N" or "k_forward_bf16<G, MODE, UNR, PNT>;grid=N": the gather-dot forward that
 * tfr_forward / tfr_eval (rows 0: float32) or tfr_bf16_forward / tfr_bf16_eval (rows 1: bf16 snapshot) launch for a model of
 * this dim and user_num at this batch, spelled as rocprofv3 prints it, and its blocks.  mode: 0 INFER, 1 TRAIN, 2 EVAL.  PNT:
 * the user rows are read by non-temporal loads (a user table above 256 MB; TFR_BF16_PNT=0|1 overrides it for the snapshot).
 * Computed on the host by the functions the launch itself uses (no model, no device).  TFR_ERR_ARG: unsupported dim, TRAIN on
 * snapshot rows, a buffer too short for the text. */
int tfr_forward_plan(int32_t dim, int64_t user_num, int32_t mode, int32_t rows, int64_t batch, char* buf, int64_t buflen);

/* LDS budget guard: static + dynamic LDS bytes per workgroup that the dispatcher requests for a shape, computed
 * on the host exactly as the launchers compute it (no device needed).  kernel: 0 k_tile_step, 1 k_seg_reduce with
 * the forward inside, 2 k_front, 3 k_mt_draw, 4 k_seg_reduce.  A gfx950 CU has 160 KB. */
int tfr_lds_bytes(int32_t kernel, int32_t dim, int64_t batch, int64_t user_num, int64_t item_num,
                  int64_t* static_bytes, int64_t* dynamic_bytes);

/* Residency guard of the small-table sweep (k_dense_tiles as a training step launches it for this shape): workgroups
 * of it that fit one CU and its scratch bytes per lane, as the runtime reports them for the loaded code, and the
 * workgroups of the launch.  The step's timing rests on the whole grid being resident at once and on no spills.
 * Needs a device. */
int tfr_sweep_residency(int32_t dim, int64_t batch, int64_t user_num, int64_t item_num,
                        int32_t* blocks_per_cu, int64_t* scratch_bytes, int64_t* grid_blocks);

/* ---- bf16 snapshot: predict and evaluate at half the row bytes - DESIGN §21 ---------------------------------------------
 *      A copy of the five tables at a point of the stream's order, private to the model: P and Q as bf16 rows, mu and
 *      the biases as float32 so that they belong to the same moment.  Training stays float32; later steps,
 *      tfr_set_table and tfr_init_tables do not change the snapshot, only another tfr_bf16_snapshot does.  tfr_destroy
 *      frees it.
 *      Element: the upper 16 bits of the float32, rounded to nearest, ties to even: (bits + 0x7FFF + ((bits >> 16) & 1))
 *      >> 16; overflow rounds to +-inf, subnormals are not flushed; NaN becomes (bits >> 16) | 0x40 (sign kept, quiet).
 *      Row: D elements at a stride of DP = 8 * ceil(D / 8) elements (tfr_bf16_row_stride), pads +0.  The layout is the
 *      library's own; tfr_bf16_get_rows reads it for debugging.
 *      Scoring widens by a shift and multiplies in float32: the products are exact, and the sum, the bias order
 *      ((dot + mu) + bu) + bi, item_abs and the evaluation formulas are tfr_forward's / tfr_eval's.
 *      tfr_bf16_snapshot builds or refreshes the copy on the model's stream and does not synchronise; memory
 *      (user_num + item_num) * DP * 2 bytes plus the bias copies; TFR_ERR_NOMEM leaves the model without a snapshot.
 *      tfr_bf16_drop frees it (TFR_OK when there is none).  The forward and eval entries return TFR_ERR_STATE before
 *      a snapshot; argument checks, batch = 0, device-pointer conventions and TFR_ERR_OOB at the next synchronising
 *      call are those of tfr_forward, tfr_forward_dev and tfr_eval.  nll_sum_out (may be NULL): the summed sigmoid
 *      cross-entropy under loss = nll, 0 otherwise.  tfr_bf16_get_rows: which = TFR_P or TFR_Q, n = rows * DP. */
int tfr_bf16_snapshot(tfr_model* m);
int tfr_bf16_drop(tfr_model* m);
int tfr_bf16_forward(tfr_model* m, const int32_t* user, const int32_t* item, int64_t batch, float* logits_out);
int tfr_bf16_forward_dev(tfr_model* m, const int32_t* d_user, const int32_t* d_item, int64_t batch, float* d_logits);
int tfr_bf16_eval(tfr_model* m, const int32_t* user, const int32_t* item, const float* rate, int64_t batch,
                  double* sum_sq_err_out, int64_t* n_equal_out, double* nll_sum_out);
int tfr_bf16_get_rows(tfr_model* m, int32_t which, uint16_t* host, int64_t n);
int tfr_bf16_row_stride(int32_t dim);
/* Top-K from the snapshot - DESIGN §24.  Everything tfr_topk / tfr_topk_dev document holds: 1 <= k <= 256, duplicate users,
 *      n_users = 0 a no-op, the exclusion CSR and its checks, item -1 / score -INFINITY past the eligible items, NaN scores
 *      never returned, order by score descending then item id ascending, the deferred TFR_ERR_OOB of the device entry, the
 *      host entry synchronises and the device entry does not, scores_out may be NULL; the launch plan is tfr_topk_plan's.
 *      Only the score differs: ((dot + mu) + bu[u]) + bi[i] on the snapshot's tables, dot = the float32 sum of the exact
 *      products of the snapshot's bf16 elements P[u,f] * Q'[i,f] (Q' = |Q| with item_abs), taken 16 features per matrix
 *      instruction (v_mfma_f32_32x32x16_bf16) in ascending order from +0.  It is not the fmaf chain of tfr_topk, and not
 *      bit-equal to tfr_bf16_forward on the same pair; it agrees with both on the snapshot's values to float32 rounding.
 *      Results are bit-identical from run to run and across batch, chunk and slice composition.  Products or partial sums
 *      in the float32 subnormal range are unspecified: the instruction may flush them.
 *      Both return TFR_ERR_STATE (naming tfr_bf16_snapshot) before a snapshot, also for n_users = 0.  They read the
 *      snapshot only: the float32 tables, training, tfr_set_table and the inverse-norm caches neither see nor move
 *      anything. */
int tfr_bf16_topk(tfr_model* m, const int32_t* users, int64_t n_users, int32_t k,
                  const int64_t* excl_indptr, const int32_t* excl_items,
                  int32_t* items_out, float* scores_out);
int tfr_bf16_topk_dev(tfr_model* m, const int32_t* d_users, int64_t n_users, int32_t k,
                      const int64_t* d_excl_indptr, const int32_t* d_excl_items,
                      int32_t* d_items_out, float* d_scores_out);
/* Held-out ranking from the snapshot - DESIGN §26.  Everything tfr_rank_items documents holds: -1 for an excluded or
 *      NaN-scored target, repeated excluded ids counted once, every check on the host before any device work, ranks_out
 *      untouched on error, n_users = 0 a no-op, it synchronises, and the ranks are bit-identical across batch, chunk, slice and
 *      row order; the launch plan is tfr_rank_plan's.  Only the keys differ: they are tfr_bf16_topk's, so for every
 *      K <= 256, 0 <= rank(t) < K exactly when t is in tfr_bf16_topk(users, K, excl)'s row, and rank(t) is its position there.
 *      TFR_ERR_STATE (naming tfr_bf16_snapshot) before a snapshot, also for n_users = 0.  It reads the snapshot only. */
int tfr_bf16_rank_items(tfr_model* m, const int32_t* users, int64_t n_users,
                        const int64_t* tgt_indptr, const int32_t* tgt_items,
                        const int64_t* excl_indptr, const int32_t* excl_items, int32_t* ranks_out);
/* Nearest neighbours from the snapshot - DESIGN §26.  Everything tfr_neighbours / tfr_neighbours_dev document holds (which,
 *      metric, k, the candidate range [lo, hi), the exclusion CSR and its checks, the query row never its own neighbour, id -1
 *      / score -INFINITY past the eligible rows, the deferred errors of the device entry, the host entry synchronises and
 *      the device entry does not) on the rows of the snapshot's Q (TFR_NB_ITEMS, Q' = |Q| with item_abs) or P (TFR_NB_USERS).
 *      dot(a, b) = the float32 sum of the exact products of the snapshot's bf16 elements, taken 16 features per matrix
 *      instruction (v_mfma_f32_32x32x16_bf16) in ascending order from +0, as in tfr_bf16_topk.  cosine(a, b) =
 *      (dot(a, b) * rn[a]) * rn[b], rn[r] = 1 / sqrtf(ss[r]) and 0 where ss[r] == 0, ss[r] = the float32 fmaf chain over f
 *      ascending from +0 of the widened elements squared (the squares are exact in float32; pads add nothing).
 *      The inverse norms are built by the first cosine query on a table and kept until the next tfr_bf16_snapshot or
 *      tfr_bf16_drop; steps, tfr_set_table and the float32 tables' own norm caches neither see nor move anything.
 *      TFR_ERR_STATE (naming tfr_bf16_snapshot) before a snapshot, also for n = 0. */
int tfr_bf16_neighbours(tfr_model* m, int32_t which, int32_t metric, const int32_t* rows, int64_t n, int32_t k,
                        const int64_t* excl_indptr, const int32_t* excl, int64_t lo, int64_t hi,
                        int32_t* ids_out, float* scores_out);
int tfr_bf16_neighbours_dev(tfr_model* m, int32_t which, int32_t metric, const int32_t* d_rows, int64_t n, int32_t k,
                            const int64_t* d_excl_indptr, const int32_t* d_excl, int64_t lo, int64_t hi,
                            int32_t* d_ids_out, float* d_scores_out);

/* ---- the FM from a bf16 snapshot: forward, resident predict / eval and top-K at half the row bytes - DESIGN §28 ----------
 *      The snapshot is the one described above, taken of an FM handle: V as bf16 rows (format, rounding, stride DP and
 *      pads as above), W and mu of the same moment in float32.  tfr_fm_train_step*, tfr_fm_train_steps_resident,
 *      tfr_fm_set and tfr_fm_init do not change it, only another tfr_fm_bf16_snapshot does; tfr_fm_destroy frees it.
 *      tfr_fm_bf16_snapshot builds or refreshes it on the model's stream and does not synchronise (n_features * DP * 2
 *      bytes plus the copy of W); tfr_fm_bf16_drop frees it (TFR_OK when there is none).  tfr_fm_bf16_get_rows copies the
 *      packed V out for debugging: n = n_features * DP.
 *      Every other entry below returns TFR_ERR_STATE (naming tfr_fm_bf16_snapshot) before a snapshot, also for
 *      n_rows = 0 or n_users = 0, and reads the snapshot only.  Argument lists, checks, device-pointer conventions and
 *      the deferred TFR_ERR_OOB of a feature id outside [0, n_features) are those of the entry without bf16 in its name.
 *      tfr_fm_bf16_forward*: the formula of tfr_fm_forward with V widened by a shift, in float32: per element
 *      xv = x * v, s += xv, q = fmaf(xv, xv, q) over the row's entries in CSR order, then sum_e (s_e^2 - q_e) over a
 *      lane's 8 elements ascending, the lanes' sums by a butterfly, y = (mu + x.W) + 0.5 * that.  Where every product
 *      and sum is exact it equals tfr_fm_forward bit for bit; results are bit-identical from run to run and do not
 *      depend on the other rows of the call.
 *      tfr_fm_bf16_predict_resident / tfr_fm_bf16_eval_binary_resident: tfr_fm_predict_resident /
 *      tfr_fm_eval_binary_resident with that forward; the metrics are computed from its predictions as theirs are.
 *      tfr_fm_bf16_topk: tfr_fm_topk's users, item range, ids relative to item_lo and exclusions with tfr_bf16_topk's
 *      score, keys, tie order and padding on the snapshot: ((dot + mu) + W[u]) + W[item_lo + i]. */
int tfr_fm_bf16_snapshot(tfr_fm* m);
int tfr_fm_bf16_drop(tfr_fm* m);
int tfr_fm_bf16_get_rows(tfr_fm* m, uint16_t* host, int64_t n);
int tfr_fm_bf16_forward(tfr_fm* m, const int64_t* indptr, const int32_t* indices, const float* data,
                        int64_t n_rows, float* out);                           /* host CSR, synchronous */
int tfr_fm_bf16_forward_dev(tfr_fm* m, const int64_t* d_indptr, const int32_t* d_indices,
                            const float* d_data, int64_t n_rows, float* d_out); /* device CSR, async */
int tfr_fm_bf16_predict_resident(tfr_fm* m, int32_t which, float* out);
int tfr_fm_bf16_eval_binary_resident(tfr_fm* m, int64_t* n_equal_out, double* nll_sum_out, double* auc_out, int64_t* n_out);
int tfr_fm_bf16_topk(tfr_fm* m, const int32_t* user_features, int64_t n_users, int64_t item_lo, int64_t item_hi,
                     int32_t k, const int64_t* excl_indptr, const int32_t* excl_items,
                     int32_t* items_out, float* scores_out);

/* ---- misc ------------------------------------------------------------------------------ */
int tfr_sync(tfr_model* m);            /* drains the stream; reports deferred TFR_ERR_OOB   */
const char* tfr_last_error(void);
int tfr_version(void);
int tfr_device_count(void);
/* Measurement yardstick (bench.py): GB/s (read + write bytes) of the library's own float4 copy kernel (one 16-byte element per
 * thread, streaming loads and stores - the fastest of the forms tools/probes/copy_bw.hip compares) over `bytes` of device
 * memory, best and mean of `reps` launches timed by HIP events.  Replaces no reference call. */
int tfr_device_copy_rate(int32_t device, int64_t bytes, int32_t reps, double* best_gbs, double* mean_gbs);

#ifdef __cplusplus
}
#endif
#endif /* TFRECOMM_H */
