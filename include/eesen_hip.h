/* eesen_hip.h -- C-ABI of libeesen_hip.so: the MI355X (gfx950) implementation of the hot path of
 * Eesen's `train-ctc-parallel` (peephole (Bi-)LSTM forward/backward, affine, softmax, CTC
 * forward-backward, SGD update) behind the reference's net/netbin operator interface.
 *
 * Plain C: opaque handles, plain pointers and sizes, int status codes.  No torch / C++ types.
 * Every entry point returns EESEN_OK (0) or a negative status; eesen_last_error() gives the message
 * of the last failure on the calling thread (the reference throws std::runtime_error from KALDI_ERR,
 * /root/reference/src/base/kaldi-error.cc:168-182; no exception crosses this boundary).
 *
 * Threading: one handle per GPU, not thread-safe per handle (the reference is single-threaded with a
 * process-global CuDevice, src/gpucompute/cuda-device.cc:846).  All work of a handle is enqueued on the
 * handle's HIP stream; entry points that return host data synchronise that stream, the others do not.
 *
 * Memory kinds: pointers marked `dev` are device pointers on the handle's GPU, `host` are host
 * pointers.  Matrices are row-major fp32 with an explicit leading dimension `ld` (elements), exactly
 * the reference's MatrixDim {rows, cols, stride} (src/gpucompute/cuda-matrixdim.h:52-56).
 * Utterance batches are time-major interleaved: row t*S + s = frame t of sequence s
 * (src/netbin/train-ctc-parallel.cc:187-193).
 */
#ifndef EESEN_HIP_H_
#define EESEN_HIP_H_

#ifdef __cplusplus
extern "C" {
#endif

#define EESEN_OK 0
#define EESEN_ERR_INVALID -1   /* bad argument / unsupported model feature (e.g. dropout tokens)   */
#define EESEN_ERR_HIP -2       /* a HIP runtime call or kernel launch failed                        */
#define EESEN_ERR_STATE -3     /* call sequence violated (e.g. Backpropagate before Propagate)      */
#define EESEN_ERR_IO -4        /* model file could not be read / written / parsed                   */
#define EESEN_ERR_COMM -5      /* the data-parallel exchange was aborted: a peer died or stalled    */

/* Layer kinds: the markers of src/net/layer.cc:37-46 that are on the hot path. */
#define EESEN_LAYER_AFFINE 1          /* <AffineTransform>  src/net/affine-trans-layer.h           */
#define EESEN_LAYER_SOFTMAX 2         /* <Softmax>          src/net/softmax-layer.h                */
#define EESEN_LAYER_LSTM_PARALLEL 3   /* <LstmParallel>     src/net/lstm-parallel-layer.h          */
#define EESEN_LAYER_BILSTM_PARALLEL 4 /* <BiLstmParallel>   src/net/bilstm-parallel-layer.h        */
#define EESEN_LAYER_SIGMOID 5         /* <Sigmoid>          src/net/sigmoid-layer.h (no parameters) */
#define EESEN_LAYER_TANH 6            /* <Tanh>             src/net/tanh-layer.h    (no parameters) */

typedef struct eesen_net eesen_net_t; /* replaces eesen::Net, src/net/net.h:37-175           */
typedef struct eesen_ctc eesen_ctc_t; /* replaces eesen::Ctc, src/net/ctc-loss.h:31-90       */
typedef struct eesen_ce eesen_ce_t;   /* replaces eesen::CE, src/net/ce-loss.h:32-77          */
typedef struct eesen_lm eesen_lm_t;   /* a token n-gram LM for eesen_ctc_decode_parallel_lm (no counterpart) */
typedef struct eesen_lex eesen_lex_t; /* a lexicon trie for eesen_ctc_decode_parallel_lex (no counterpart)   */

/* ---- library / device ------------------------------------------------------------------------ */
const char* eesen_last_error(void);
const char* eesen_version(void);
/* replaces CuDevice::Instantiate().SelectGpuId (src/gpucompute/cuda-device.cc:73-140): number of
 * visible HIP devices (0 is not an error here; creating a handle then fails loudly). */
int eesen_device_count(int* count);

/* Arithmetic of the dense contractions outside the time recurrence (what the reference sends to cublasSgemm through
 * CuMatrixBase::AddMatMat, src/gpucompute/cuda-matrix.cc:604-639), process-wide:
 *   0  f32-input MFMA (v_mfma_f32_32x32x2_f32): bit-for-bit a k-ordered fp32 fmaf chain, at the f32 vector rate;
 *   1  3-way bf16 split: every fp32 operand is EXACTLY hi + mid + lo (three bf16), six of the nine cross products run on
 *      v_mfma_f32_32x32x16_bf16 with fp32 accumulation; error <= 2^-23 |a*b| per product, i.e. fp32-GEMM class, at 2.67x the
 *      f32 matrix rate (gfx950 runs f32 MFMA at 1/16 of the bf16 rate and has no TF32 form);
 *   2  two fp16 planes (round 6, the default): every fp32 operand is hi + lo (fp16, round to nearest at both levels: equal to
 *      the value to within 2^-22), each row of op(A) / column of op(B) scaled by the exact power of two its own largest magnitude
 *      asks for (measured on the device), three of the four cross products on v_mfma_f32_32x32x16_f16 with fp32 accumulation;
 *      error <= 3 * 2^-22 |a*b| per product (the "3xTF32" arithmetic; measured against fp64 equal to modes 0 and 1,
 *      tests/test_gpu_gemm.py) at 1.58x the rate of mode 1;
 *  -1  follow the environment (EESEN_GEMM_MODE=f32|split|half; half when unset), the initial state. */
int eesen_set_gemm_mode(int mode);
int eesen_get_gemm_mode(int* mode);

/* ---- Net: construction, model I/O ------------------------------------------------------------ */
/* New empty net on `device`.  `stream` is a hipStream_t to enqueue on (e.g. the caller framework's
 * current stream) or NULL for the device's default stream.  A Net and the Ctc it feeds must share a
 * stream (the reference has one implicit stream for everything).  A handle is not thread-safe, and the recurrence
 * kernels are cooperative launches that want every CU of the device: two Nets on the same device must not run
 * Propagate / Backpropagate CONCURRENTLY on different streams (each would hold half the CUs and wait for the rest until
 * its spin bound raises EESEN_ERR_HIP); on one stream, or one after the other, any number of handles coexist. */
int eesen_net_create(int device, void* stream, eesen_net_t** out);
int eesen_net_destroy(eesen_net_t* net);
/* Net::AppendLayer (src/net/net.cc:197-205) with the layer header of src/net/layer.cc:138-222:
 * in_dim = <InputDim>, out_dim = <CellDim> (LSTM kinds: 2H for BiLstm, H for Lstm) or <OutputDim>. */
int eesen_net_add_layer(eesen_net_t* net, int kind, int in_dim, int out_dim,
                        float learn_rate_coef, float max_grad);
/* Allocates parameters (zero) + optimiser state; must follow the last add_layer. */
int eesen_net_finalize(eesen_net_t* net);
/* Net::Read (src/net/net.cc:279-309): parse a Kaldi-stream <Nnet> file (text or \0B binary), build
 * the layers and upload the weights (and the Adagrad/RMSProp accumulators when the file carries them; the nine dropout
 * options of a BiLstm layer are kept, see the dropout section below).  Fails (EESEN_ERR_INVALID) on layer kinds outside
 * the list above.  Resets learn_rate to 0 as the reference does (net.cc:294). */
int eesen_net_read(eesen_net_t* net, const char* path);
/* Net::Write (src/net/net.cc:325-334), same byte format as the reference for these layer kinds. */
int eesen_net_write(eesen_net_t* net, const char* path, int binary);

int eesen_net_num_layers(eesen_net_t* net, int* n);
int eesen_net_layer_info(eesen_net_t* net, int idx, int* kind, int* in_dim, int* out_dim,
                         float* learn_rate_coef, float* max_grad);
/* Layer::TypeToMarker (src/net/layer.cc:68-79): the marker token of layer idx as its model file carries it
 * ("<BiLstmParallel>", "<BiLstm>", "<AffineTransform>", ...), NUL-terminated into buf[cap]. */
int eesen_net_layer_marker(eesen_net_t* net, int idx, char* buf, int cap);
/* What Net::Info / Net::InfoGradient print per tensor (src/net/net.cc:336-385 through MomentStatistics,
 * src/net/utils-functions.h:50-82): {min, max, mean, variance, skewness, kurtosis} of each tensor of `layer`, in the order
 * of the layer's own Info() (bilstm-layer.h:496-560: W_x, W_m, bias, p_i, p_f, p_o forward, then backward; lstm-layer.h:175-196;
 * affine-trans-layer.h:145-159: linearity, bias).  which: 0 = the parameters (Info), 1 = the momentum buffers *_corr_
 * (InfoGradient), 2 = the Adagrad / RMSProp accumulators *_corr_accu.  Computed on the device (two reduction passes per
 * tensor, fp64 accumulation).  out6_host: [cap_tensors x 6] doubles or NULL (count only); *n_tensors = tensors of the layer
 * (0 for layers without parameters).  Synchronises. */
int eesen_net_tensor_moments(eesen_net_t* net, int which, int layer, double* out6_host, int cap_tensors, int* n_tensors);
int eesen_net_input_dim(eesen_net_t* net, int* dim);   /* Net::InputDim  net.cc:139-142 */
int eesen_net_output_dim(eesen_net_t* net, int* dim);  /* Net::OutputDim net.cc:134-137 */
int eesen_net_num_params(eesen_net_t* net, long* n);   /* Net::NumParams net.cc:163-172 */
/* Net::GetParams / SetParams order (src/net/net.cc:181-195): per trainable layer its tensors in
 * model-file order, each row-major and dense.  host pointers, n = num_params. */
int eesen_net_get_params(eesen_net_t* net, float* host_flat, long n);
int eesen_net_set_params(eesen_net_t* net, const float* host_flat, long n);

/* ---- Net: training options (src/net/train-opts.h:29-62, net.h:147-161) ------------------------- */
int eesen_net_set_train_options(eesen_net_t* net, float learn_rate, float momentum);
/* Net::SetUpdateAlgorithm (src/net/net.cc:481-497): "SGD" (default), "Adagrad", "RMSProp" (trainable-layer.h:65-114). */
int eesen_net_set_update_algorithm(eesen_net_t* net, const char* name);
/* NetTrainOptions::adagrad_epsilon (1e-6) and rmsprop_rho (0.9) (train-opts.h:33-42). */
int eesen_net_set_adaptive_options(eesen_net_t* net, float adagrad_epsilon, float rmsprop_rho);
/* The squared-gradient accumulators (*_corr_accu, bilstm-layer.h:1098-1124) in Net::GetParams order; they are what
 * <BiLstmAccus>/<LstmAccus>/<AffineAccus> carry in a model file. Zero until an adaptive rule ran or a file held them. */
int eesen_net_get_accumulators(eesen_net_t* net, float* host_flat, long n);
int eesen_net_set_accumulators(eesen_net_t* net, const float* host_flat, long n);
/* Net::SetSeqLengths (net.h:157): frame count of each of the S parallel sequences. host pointer. */
int eesen_net_set_seq_lengths(eesen_net_t* net, const int* lens, int S);

/* ---- Net: forward / backward / update -------------------------------------------------------- */
/* Net::Propagate (src/net/net.cc:67-86).  in: [rows x input_dim], rows = T*S, `in_is_device` selects
 * the memory kind (the reference trainer hands a host Matrix that the CuMatrix ctor uploads,
 * train-ctc-parallel.cc:198).  The output stays on the device and is owned by the handle:
 * *out_dev -> [rows x *out_cols] fp32 with leading dimension *out_ld, valid until the next Propagate.
 * Rows t >= len[s] hold unspecified values (the reference computes on padding too; nothing reads them). */
int eesen_net_propagate(eesen_net_t* net, const float* in, int rows, int in_ld, int in_is_device,
                        const float** out_dev, int* out_cols, int* out_ld);
/* Copy the last Propagate output to the host ([rows x output_dim], dense). Synchronises. */
int eesen_net_get_output(eesen_net_t* net, float* host_out, long n);

/* Net::Backpropagate minus Update (src/net/net.cc:88-108, with :101-104 split out so that a
 * data-parallel gradient exchange can run between the two).  out_diff_dev: [rows x output_dim]
 * device matrix, d(-ln p)/d(logits) as Ctc::EvalParallel returns it.  After the call every
 * parameter has its FRESH gradient (sum over frames, momentum not yet folded in) in the gradient
 * buffer.  in_diff_dev: optional [rows x input_dim] device matrix (NULL in the trainer,
 * train-ctc-parallel.cc:207). */
int eesen_net_backpropagate(eesen_net_t* net, const float* out_diff_dev, int out_diff_ld,
                            float* in_diff_dev, int in_diff_ld);
/* The contiguous device buffer of fresh gradients of ALL parameters (n floats, library-internal
 * tensor layout, identical on every rank): the payload of the data-parallel all-reduce(SUM) that
 * replaces comm_avg_weights (src/net/communicator.h:39-119). */
int eesen_net_grad_buffer(eesen_net_t* net, float** dev_ptr, long* n);
/* Fresh gradients in Net::GetParams order on the host (debug / parity accessor; the reference keeps
 * *_corr_ protected, src/net/bilstm-layer.h:1076-1096). Synchronises. */
int eesen_net_get_grads(eesen_net_t* net, float* host_flat, long n);
/* TrainableLayer::Update for every layer, SGD rule (src/net/bilstm-layer.h:846-883,
 * affine-trans-layer.h:174-195): corr = momentum*corr + fresh; clip corr to +-max_grad if
 * max_grad > 0; param -= learn_rate*learn_rate_coef*corr. */
int eesen_net_update(eesen_net_t* net);
/* BASELINE config 4's "bf16 forward / fp32 CTC accumulate" variant (no counterpart in the reference, whose BaseFloat is float,
 * src/base/kaldi-types.h:26-30).  mode 1: the whole forward pass multiplies in bf16 with fp32 accumulation --
 *   (a) the GEMMs of Propagate (input->gates, affine / projection) round both operands to nearest-even bf16 and run ONE
 *       v_mfma_f32_32x32x16_bf16 product;
 *   (b) the forward TIME RECURRENCE (the loop of src/net/bilstm-parallel-layer.h:112-149,165-204) keeps W_m as TWO bf16 planes
 *       (hi + lo: 17 significant bits), rounds m_t to ONE bf16 plane, at the cell write into the kernel's exchange buffer, and
 *       forms m_{t-1} W_m^T on
 *       v_mfma_f32_16x16x32_bf16 (layers with H a multiple of 256 up to 1024 cells per direction, no recurrent dropout; other
 *       layers keep the fp32 recurrence).  Gate pre-activations, cell state, activations, and everything stored for the
 *       backward pass stay fp32;
 * softmax, CTC, the whole backward pass and the update stay fp32.  mode 2: (a) only.
 * (Up to round 3 of this library value 1 meant (a) only; since round 4 it also selects (b), and (a) alone is value 2.)
 * mode 0 (default): fp32 everywhere.  Distances: tests/test_gpu_gemm.py::test_bf16_forward_variant against this library's fp32
 * path; against THE REFERENCE at BASELINE config 4's full size: tests/test_gpu_reference_fullsize.py, profiles/parity_cfg4.json. */
int eesen_net_set_forward_precision(eesen_net_t* net, int mode);
/* Debug / test accessor: how many LSTM layers of the last Propagate ran their recurrence on the bf16 kernel of (b). */
int eesen_net_bf16_recurrence_layers(eesen_net_t* net, int* layers);
/* Debug / test accessor: out4 = {LSTM layers, layers whose forward time loop ran as ONE cooperative launch per sequence
 * window (lstm_persistent.hip), layers whose backward time loop did} for the last Propagate / Backpropagate (the rest
 * took the one-launch-per-step kernels), and the number of recoveries so far.  A recovery: a cooperative recurrence
 * kernel whose bounded spin gave up (its workgroups were not all resident -- GPU shared or preempted) raises a device
 * word; the update kernels of that step see it and leave the model untouched, and the handle continues on the per-step
 * kernels with a WARNING on stderr.  With a communicator attached the other ranks do apply their step: the failed rank's
 * gradients then enter the all-reduce as zeros (decided on the device) and it applies the same summed update, so the ranks' models
 * stay identical and the run only loses that rank's share of the minibatches in flight. */
int eesen_net_recurrence_info(eesen_net_t* net, int* out4);
/* What WILL run the current minibatch shape (call after eesen_net_set_seq_lengths), as one JSON object: per LSTM layer the forward
 * and backward recurrence plans -- kernel instantiation, sequences / units per workgroup, grid, launches per pass, registers per
 * lane and LDS bytes of the instantiation, registers per SIMD lane its grid leaves free on a CU -- and the schedule decisions that
 * follow from them: for a layer behind an LSTM layer which schedule its input GEMM takes around the forward recurrences ("input_gemm": whole; gated; the
 * middle rows early and both ends, or only the needed quadrants, in front of the recurrence), weight-gradient GEMMs on the side
 * stream or not, the exchange schedule with a communicator attached.  The
 * launchers execute exactly these plans (one selection function per pass, rec_plan.cpp: lstm_fwd_plan / lstm_bwd_plan).
 * Diagnostic; the reference has no counterpart (its kernels are chosen at compile time, src/gpucompute/cuda-kernels.cu). */
int eesen_net_plan_string(eesen_net_t* net, char* json, int cap);
/* Test hook: stores `value` into that device word on the handle's stream, as a kernel that gave up would (1: a recurrence
 * kernel's bounded spin, 2: the side stream's wait for a forward milestone), so that the recovery paths can be exercised. */
int eesen_net_debug_set_error_word(eesen_net_t* net, unsigned value);
/* Test hook, read-only: one intermediate buffer of LSTM layer `layer` as the last Propagate / Backpropagate left it.  which: 0 the
 * gate activations (they overwrite the pre-activations G), 1 the cell state c, 2 the unmasked output m (what the recurrence and the
 * W_m gradient read), 3 the gate gradients DG of the last Backpropagate.  The call drains the handle's stream and the side stream
 * and copies the T * S interior rows (row t * S + s; the boundary blocks t = -1 and t = T are left out) into `host`, in the MODEL
 * FILE's column order: per direction the gate blocks g, i, f, o of H columns each (the order of the W_x rows) for 0 and 3, H cells
 * for 1 and 2.  *rows and *cols receive the shape; with host == NULL nothing else happens, otherwise cap_floats >= rows * cols.
 * EESEN_ERR_STATE: not an LSTM layer, nothing propagated, or (3) no Backpropagate since the last Propagate / a lower layer has
 * reused the layer's gate-gradient buffer (two buffers alternate between the LSTM layers).  It changes no schedule; no tool calls it. */
int eesen_net_debug_layer_buffer(eesen_net_t* net, int layer, int which, float* host, long cap_floats, int* rows, int* cols);
/* Block until everything enqueued on the handle's stream has finished. */
int eesen_net_synchronize(eesen_net_t* net);
/* Seconds spent (HIP events on the handle's stream) in the phases of the last step, for bench.py:
 * out[0]=input GEMMs, [1]=recurrence fwd, [2]=affine+softmax, [3]=recurrence bwd, [4]=gradient GEMMs
 * and reductions, [5]=update.  Enabled by eesen_net_set_profiling(net, 1); with 2 the timers ACCUMULATE over all steps
 * since the last eesen_net_get_phase_times, so a multi-step region needs no host synchronisation per step. */
int eesen_net_set_profiling(eesen_net_t* net, int on);
int eesen_net_get_phase_times(eesen_net_t* net, float* out6);
/* The individual timed spans behind those sums, in the order they were recorded: phases[i] (index as above) and seconds[i]
 * of span i, up to `cap`; *n = spans recorded since the last eesen_net_get_phase_times.  One span per kernel group of a
 * layer (e.g. one per layer and step for the recurrences, top layer first in the backward pass), so a caller can separate
 * the launch that runs alone on the chip from those that share it with side-stream work.  Call BEFORE get_phase_times.
 * With a communicator attached two more span kinds appear here (they are not part of out6): phase 6 = one gradient bucket's
 * all-reduce on the communicator's stream (from "bucket ready and stream free" to the end of the collective; in the order of
 * eesen_net_bucket_order), phase 7 = the time the compute stream waited for one bucket inside eesen_net_update -- the part of
 * the exchange the lower layers' backward pass did not hide. */
int eesen_net_get_phase_spans(eesen_net_t* net, int* phases, float* seconds, int cap, int* n);

/* ---- data-parallel exchange: one process per GPU, RCCL over xGMI ------------------------------------------------------
 * Replaces the reference's multi-job mode (--num-jobs / --job-id / --utts-per-avg, src/netbin/train-ctc-parallel.cc:208-235):
 * comm_avg_weights (src/net/communicator.h:39-119) averages whole MODELS through files every few hundred utterances and
 * comm_touch_done (:121-170) merges the error counts through "done" files.  Here every rank runs the same Net on its own
 * utterances and the FRESH gradients (sums over frames) are summed over the ranks every minibatch, so that N ranks x S
 * utterances equal one process with --num-sequence = N*S (momentum and clipping act on the summed gradient).
 *
 * Rendezvous: rank 0 draws the 128-byte RCCL unique id (eesen_comm_get_unique_id) and hands it to the other ranks --
 * through any channel the host has (eesen_comm_create), or through the library's own TCP hand-out
 * (eesen_comm_create_tcp: rank 0 listens on addr:port, the others connect, retrying until `timeout_s`).
 * eesen_comm_exchange is that hand-out on its own (any <= 4 KB blob; needs no GPU). */
typedef struct eesen_comm eesen_comm_t;
int eesen_comm_get_unique_id(char* id128);
int eesen_comm_exchange(const char* addr, int port, int rank, int world, char* buf, int nbytes, int timeout_s);
int eesen_comm_create(int device, const char* id128, int rank, int world, eesen_comm_t** out);
int eesen_comm_create_tcp(int device, const char* addr, int port, int rank, int world, int timeout_s, eesen_comm_t** out);
int eesen_comm_destroy(eesen_comm_t* comm);
int eesen_comm_info(eesen_comm_t* comm, int* rank, int* world);
/* What the communicator really is, as one JSON object -- COLLECTIVE: every rank calls it (it gathers one word per rank).
 * {library: path the dynamic linker resolved, rccl_version: ncclGetVersion, stand_in: the tests' stand-in and not RCCL,
 *  rank / world: as created, world_seen / rank_seen / device_seen: ncclCommCount / ncclCommUserRank / ncclCommCuDevice,
 *  devices: [hosthash/PCI bus id of every rank's GPU], distinct_devices, ranks_share_devices}.
 * The reference's multi-job mode has no such thing (its jobs only meet through files, src/net/communicator.h:39-170); a
 * collective-based exchange owes its operator the answer to "did N ranks on N distinct GPUs really meet". */
int eesen_comm_describe(eesen_comm_t* comm, char* json, int cap);
/* Sum (op 0) or max (op 1) of n <= 64 host doubles over the ranks, in place; blocks.  Carries the statistics the
 * reference merges through done-files (sum ln p, error / reference tokens, frames), "does any rank still have a
 * minibatch", and doubles as a barrier. */
int eesen_comm_allreduce_host(eesen_comm_t* comm, double* values, int n, int op);
/* Attach a communicator to a Net (NULL detaches).  From then on eesen_net_backpropagate sums every layer's fresh
 * gradients over the ranks -- one all-reduce(SUM, fp32) per trainable layer, issued on the communicator's own stream as
 * soon as that layer's weight-gradient kernels are enqueued, i.e. where the reference updates the layer
 * (src/net/net.cc:98-104), so the exchange of the upper layers runs under the backward pass of the lower ones -- and
 * eesen_net_update waits bucket by bucket.  Every rank must call the same sequence of backpropagate / update. */
int eesen_net_set_comm(eesen_net_t* net, eesen_comm_t* comm);
/* The same exchange as ONE all-reduce of the whole gradient buffer on the Net's stream, for hosts that keep the
 * communicator detached: call between eesen_net_backpropagate and eesen_net_update. */
int eesen_net_allreduce_grads(eesen_net_t* net, eesen_comm_t* comm);
/* Jobs with different numbers of minibatches (the reference's sub-jobs simply stop when job 1 has finished,
 * src/net/communicator.h:104-112): a rank that has run out of minibatches while others have not keeps stepping with
 *   eesen_net_backpropagate_zero (zero gradient, the attached communicator's per-layer all-reduces in the order a real
 *   Backpropagate issues them) + eesen_net_update + eesen_net_live_ranks
 * until live_ranks reports 0.  One float rides with the top layer's gradient bucket: 1 from every rank whose step was a real
 * eesen_net_backpropagate, 0 from the others; *live is its sum over the ranks for the last step issued (blocks until that
 * bucket has arrived).  A step in which NO rank was live -- the closing round, which all ranks take together -- leaves the
 * model untouched (the update kernels read the word on the device), so N ranks with uneven shards still equal one process
 * on the union of their minibatches.  Ranks that still train never need to ask. */
int eesen_net_backpropagate_zero(eesen_net_t* net);
int eesen_net_live_ranks(eesen_net_t* net, int* live);
/* A peer that dies leaves the others' collectives spinning.  Every communicator runs a watchdog: a collective that has not
 * completed EESEN_COMM_TIMEOUT_S (default 600) seconds after it was issued is aborted (ncclCommAbort), every blocked wait
 * returns, and every later call on the communicator or a net attached to it fails with EESEN_ERR_COMM. */
/* Debug / test accessor: the layer indices whose buckets the last Backpropagate issued, in issue order. */
int eesen_net_bucket_order(eesen_net_t* net, int* layers_out, int cap, int* n);
/* hipDeviceSynchronize of `device` (bench.py brackets its timed region with it). */
int eesen_device_synchronize(int device);

/* ---- Ctc (src/net/ctc-loss.h:31-90) ------------------------------------------------------------ */
int eesen_ctc_create(int device, void* stream, eesen_ctc_t** out);
int eesen_ctc_destroy(eesen_ctc_t* ctc);
/* Ctc::EvalParallel (src/net/ctc-loss.cc:101-194).  net_out_dev: [T*S x K] softmax outputs (device),
 * frame_num_utt: host int[S]; labels in CSR form on the host: label_off int[S+1], label_ids (no
 * blanks, blank id is 0).  Writes diff_dev [T*S x K] (device, ld given) = d(-ln p)/d(logits), zero
 * on rows t >= frame_num_utt[s]; pzx_host (may be NULL: then nothing waits for the device and ln p joins the
 * objective sum once it has arrived): ln p(z|x) per sequence.  Accumulates the
 * objective / frame counters reported by eesen_ctc_report.  Every sequence needs >= 1 label and a
 * feasible alignment is the caller's business (ln p ~ -1e30 otherwise, as in the reference).
 * Limits (EESEN_ERR_INVALID beyond them; the reference has none): at most 2047 labels per sequence -- expanded label sequences
 * of up to 4096 lattice positions -- and at most 20480 classes (5120 before round 6's closing change). */
int eesen_ctc_eval_parallel(eesen_ctc_t* ctc, const int* frame_num_utt, int S, const float* net_out_dev,
                            int rows, int K, int ld, const int* label_ids, const int* label_off,
                            float* diff_dev, int diff_ld, float* pzx_host);
/* Ctc::ErrorRateMSeq (ctc-loss.cc:235-298): greedy decode (argmax on the device, collapse repeats,
 * drop blanks) and Levenshtein distance against the references (host).  Accumulates error / ref
 * token counts; also returns this call's counts.  With num_err == num_ref == NULL the call only ENQUEUES the argmax
 * and the copy of the ids: the host part runs at the next call / eesen_ctc_stats, under the device's backward pass
 * (the reference's call returns void and only accumulates). */
int eesen_ctc_error_rate_mseq(eesen_ctc_t* ctc, const int* frame_num_utt, int S, const float* net_out_dev,
                              int rows, int K, int ld, const int* label_ids, const int* label_off,
                              int* num_err, int* num_ref);
/* --sequence-out-file of the trainer (src/netbin/train-ctc-parallel.cc:53-54,134-137; written by Ctc::ErrorRateMSeq,
 * ctc-loss.cc:247-250,282-291): every later eesen_ctc_error_rate_mseq appends one line per utterance,
 * `utt | <label> <frame> <probability> | ...` for the greedy-decoded sequence.  The file is removed first, as the
 * reference's trainer does; NULL or "" switches the output off. */
int eesen_ctc_set_sequence_out_file(eesen_ctc_t* ctc, const char* path);
/* Guard the statistics against a timed-out forward pass.  A cooperative recurrence kernel whose bounded spin gave up leaves
 * garbage activations and raises a device word (eesen_net_recurrence_info); the Net recovers on its own, but a minibatch the
 * host had already handed to the Ctc would fold a garbage ln p and garbage decodes into the objective and TOKEN_ACCURACY.  With
 * a guard the word's value travels back with every minibatch's results, and a minibatch computed while it was set is dropped
 * from ALL running totals (eesen_ctc_dropped counts them; one WARNING on stderr) and the ln p values eesen_ctc_eval_parallel hands
 * back for it read NaN.  The Ctc and the Net must share device and stream (the word is read in stream order); either may be
 * destroyed first.  net == NULL removes the guard. */
int eesen_ctc_set_guard(eesen_ctc_t* ctc, eesen_net_t* net);
int eesen_ctc_dropped(eesen_ctc_t* ctc, long* minibatches);
/* Running totals: Ctc::NumErrorTokens/NumRefTokens (ctc-loss.h:58-59) and the sums behind
 * Ctc::Report (ctc-loss.cc:300-308): obj = sum of ln p, sequences, frames. */
int eesen_ctc_stats(eesen_ctc_t* ctc, double* obj_sum, long* sequences, long* frames, long* err_tokens,
                    long* ref_tokens);
/* Debug / parity accessor: alpha and beta of the last EvalParallel in the reference's layout
 * [T*S x L'] (row t*S+s, L' = 2*max_U+1), host pointers, either may be NULL. Cells the reference
 * leaves at -1e30 (padding) read -1e30. */
int eesen_ctc_get_alpha_beta(eesen_ctc_t* ctc, float* alpha_host, float* beta_host, int* Lprime);
/* seconds of the last EvalParallel's device work (HIP events): out[0]=log, [1]=alpha/beta sweep, [2]=error+jacobian.
 * eesen_ctc_set_profiling(ctc, 2): the spans of ALL calls since the last read are summed instead, so that a timed
 * multi-step region needs no host synchronisation per step (0 = back to last-call timing). */
int eesen_ctc_set_profiling(eesen_ctc_t* ctc, int mode);
int eesen_ctc_get_phase_times(eesen_ctc_t* ctc, float* out3);
/* Best-path (Viterbi) alignment of every utterance against its labels: which lattice position, hence which class, each frame
 * belongs to on the single most likely path.  The reference has no such call: it aligns one utterance at a time through a TLG
 * graph and the WFST decoder (asr_egs/wsj/steps/align_ctc_single_utt.sh:67-85).  Arguments as eesen_ctc_eval_parallel;
 * scores_dev [T*S x K] (device, ld >= K) holds posteriors (is_log == 0: the call takes the logarithm itself) or log-domain scores
 * (is_log != 0: e.g. what eesen_op_log_sub_prior left, prior-scaled log-likelihoods).  With l' the labels interleaved with blanks
 * (L' = 2U+1 positions, blank = 0) and s_t(k) the log-score of class k at frame t:
 *   delta_0(0) = s_0(l'_0), delta_0(1) = s_0(l'_1), delta_0(j >= 2) = -1e30
 *   delta_t(j) = s_t(l'_j) + max(delta_{t-1}(j), delta_{t-1}(j-1), [delta_{t-1}(j-2) iff j odd and l'_j != l'_{j-2}])
 *   j_end = argmax(delta_{n-1}(L'-1), delta_{n-1}(L'-2)), score = delta_{n-1}(j_end), traced back to t = 0.
 * Tie rule (part of the interface): among equal predecessors the smallest move wins -- stay, then j-1, then j-2 -- and at the end
 * the final blank L'-1 wins over L'-2.  The additions run in path order in fp32, so two paths that emit the same classes have
 * bit-identical scores and the rule decides between them.
 * Host outputs: ali_host [rows] the class id l'_{j_t} at row t*S + s (the row order of the scores and of eesen_ce_eval_parallel's
 * targets), pos_host [rows] (may be NULL) the lattice position j_t, score_host [S].  Rows t >= frame_num_utt[s] read -1.
 * An utterance without a feasible path -- fewer frames than labels + adjacent repeats, no frames, best final delta <= -1e29 --
 * is a result, not an error: score -1e30 and -1 in every row; the other utterances are not affected.  The shortest feasible
 * length (labels + adjacent repeats frames: one path, ending on the last label) is an ordinary case.
 * Restrictions as eesen_ctc_eval_parallel (EESEN_ERR_INVALID): >= 1 label per utterance, L' <= 4096, labels in [0, K), ld >= K.
 * The objective / error statistics are not touched; the lattice buffers of the last eesen_ctc_eval_parallel are borrowed
 * (eesen_ctc_get_alpha_beta afterwards reads this call's delta rows).  With a guard (eesen_ctc_set_guard) a minibatch computed
 * while the Net's recurrence error word was set returns score = NaN and ali = pos = -1.  The call waits for its results. */
int eesen_ctc_align_parallel(eesen_ctc_t* ctc, const int* frame_num_utt, int S, const float* scores_dev, int rows, int K, int ld,
                             int is_log, const int* label_ids, const int* label_off,
                             int* ali_host /*rows*/, int* pos_host /*rows or NULL*/, float* score_host /*S*/);
/* seconds of the last eesen_ctc_align_parallel's device work: out[0]=log (is_log == 0), [1]=max-plus sweep, [2]=traceback;
 * summed over all calls since the last read under eesen_ctc_set_profiling(ctc, 2). */
int eesen_ctc_get_align_times(eesen_ctc_t* ctc, float* out3);
/* Lexicon-free CTC prefix beam search of every utterance: the most probable LABELLING (a sum over paths, where the greedy collapse of
 * eesen_ctc_error_rate_mseq keeps one path), its log-probability, and an N-best list.  The reference has no such call: it decodes one
 * utterance per process through a TLG graph and its WFST decoder.  frame_num_utt, S, scores_dev, rows, K, ld, is_log as
 * eesen_ctc_align_parallel (is_log != 0: e.g. what eesen_op_log_sub_prior left).  Blank = class 0; every log-score is clamped from
 * below at -1e30 on load.  The computation, per utterance of n frames, with beam = B, max_classes = C, nbest = N:
 *   candidates of a frame: the C' = min(C, K-1) non-blank classes with the largest s_t(k), ties to the smaller class id;
 *   an entry is (prefix, lb, lnb): the log-mass of the paths that spell the prefix and end in blank / in its last label e; the beam
 *   starts as the empty prefix with lb = 0, lnb = -1e30; with tot = logadd(lb, lnb), at frame t
 *     stay of p:        lb' = s_t(0) + tot,  lnb' = s_t(e) + lnb  (-1e30 for the empty prefix)
 *     extension p + c:  lb' = -1e30,         lnb' = s_t(c) + (c == e ? lb : tot)      for every candidate class c
 *     merge:            if p + c is itself in the beam as q, its lnb' is log-added into q's stay and it is no candidate of its own;
 *   candidates whose total logadd(lb', lnb') is <= -1e29 are dead; the B largest totals survive.
 * The order is total and part of the interface: higher total first; on equal totals stays before extensions, stays by previous
 * rank, extensions by the parent's rank, then by class id.  logadd(a, b) = max + log(1 + exp(min - max)) in fp32.
 * Host outputs, with T = rows / S: hyp_host [S][nbest][T] int32, the labels (blank-free) of the min(nbest, live entries) best
 * entries after frame n-1, best first, -1 beyond each length; hyp_len_host [S][nbest], -1 beyond the returned count; score_host
 * [S][nbest] the totals, -1e30 beyond it.  n == 0 returns the empty labelling with score 0.  A beam that dies entirely (possible only
 * with is_log input, e.g. an all -inf row) returns count 0 for that utterance and leaves the others untouched.
 * Limits (EESEN_ERR_INVALID): 1 <= beam <= 64, 1 <= max_classes <= 64, beam * max_classes <= 2048, 1 <= nbest <= beam, K >= 2,
 * ld >= K, S * (1 + T * beam) <= 2^30.
 * The objective / error statistics and the lattices of the last eesen_ctc_eval_parallel are not touched.  With a guard
 * (eesen_ctc_set_guard) a minibatch computed while the Net's recurrence error word was set returns score = NaN and hyp_len = -1.
 * The call waits for its results. */
int eesen_ctc_decode_parallel(eesen_ctc_t* ctc, const int* frame_num_utt, int S, const float* scores_dev, int rows, int K, int ld,
                              int is_log, int beam, int max_classes, int nbest,
                              int* hyp_host /*S*nbest*T*/, int* hyp_len_host /*S*nbest*/, float* score_host /*S*nbest*/);
/* seconds of the last eesen_ctc_decode_parallel's device work: out[0]=candidate classes (with the logarithm when is_log == 0),
 * [1]=beam, [2]=hypotheses; summed over all calls since the last read under eesen_ctc_set_profiling(ctc, 2). */
int eesen_ctc_get_decode_times(eesen_ctc_t* ctc, float* out3);
/* The candidate classes the last eesen_ctc_decode_parallel selected (tests): ids_host / scores_host [rows][C'] in ascending id order,
 * blank_host [rows], *num_classes = C'; any pointer may be NULL.  Rows beyond an utterance's length read -1 / -1e30. */
int eesen_ctc_get_decode_candidates(eesen_ctc_t* ctc, int* ids_host, float* scores_host, float* blank_host, int* num_classes);

/* ---- token n-gram LM, fused into the prefix beam search (INTEGRATION.md "Decoding", "LM fusion") ---------------------------------
 * An ARPA file whose words are the net's own tokens, compiled on the host into a deterministic backoff automaton.  units_path: the
 * recipes' units.txt (`symbol id` per line, ids in [1, K), blank 0 implied), or NULL: the ARPA's words are decimal class ids then.
 * A word is looked up in the units table first (the recipes have a unit spelled <UNK>), then as <s>, </s> and the LM's unknown word
 * <unk>; any other word is an error that names it.  N-grams that predict <s> are ignored.  Values are log10 in the file and are
 * stored as fp32 natural logarithms, float(v * ln 10).  Every class 1 .. K-1 needs a unigram; one without takes <unk>'s, and without
 * <unk> creation fails and names the class.  The file need not be suffix-closed.
 * The automaton: state 0 is the empty context with exactly K-1 arcs; one state per listed n-gram of order < N that does not end in
 * </s> or <unk>; the start state is <s>'s (0 without <s>).  An arc of state h for class c carries (w, next), next = the longest
 * suffix of h c that is a state; a state carries (bo_w, bo_next) (bo_w = 0 where the file gives none) and final = ln P(</s> | state)
 * with the backoffs resolved (0 when the file has no </s>).
 *   lm_step(state, c): acc = 0; while the state has no arc for c: acc += bo_w, state = bo_next; return (acc + w, next)   -- in fp32
 * Limits (EESEN_ERR_INVALID, the message names the limit): order 1..8, states and arcs below 2^31.  A malformed file (no \data\
 * section, a section whose count disagrees with the header, a line whose word count does not fit its section, a non-numeric value,
 * an n-gram whose (n-1)-word prefix is not listed, an n-gram listed twice) is EESEN_ERR_INVALID with the file and line.  No device work here: the tables
 * are uploaded by the first eesen_ctc_decode_parallel_lm of a Ctc that uses the model. */
int eesen_lm_create_from_arpa(const char* arpa_path, const char* units_path /*or NULL*/, int K, eesen_lm_t** lm);
int eesen_lm_destroy(eesen_lm_t* lm);
int eesen_lm_info(eesen_lm_t* lm, int* order, int* states, int* arcs, int* has_eos);   /* any pointer may be NULL */
int eesen_lm_step(eesen_lm_t* lm, int state, int c, float* w, int* next);
int eesen_lm_start(eesen_lm_t* lm, int* state);
int eesen_lm_final(eesen_lm_t* lm, int state, float* w);
/* ln P_lm(labels [, </s>]) from the start state: the automaton walked in fp64 on the stored fp32 weights; *abs_sum_f64 (may be
 * NULL) the sum of the magnitudes of the weights on the walk.  use_eos on a model without </s> is EESEN_ERR_INVALID. */
int eesen_lm_score(eesen_lm_t* lm, const int* labels, int n, int use_eos, double* logprob_f64, double* abs_sum_f64);
/* eesen_ctc_decode_parallel with the LM fused in (shallow fusion): lm_weight = alpha, insertion_bonus = beta in nats per label.
 * Only this changes in the computation stated there: an entry also carries its LM state and lmsum, the unweighted ln P_lm of its
 * prefix (the empty prefix: the start state, 0).  For the extension p + c: (w, next) = lm_step(state_p, c), g = alpha * w + beta,
 * lnb' = (s_t(c) + g) + (c == e ? lb : tot) with both sums clamped at -1e30 -- alpha = beta = 0 reproduces the unfused bits --,
 * the new entry has state next and lmsum_p + w.  A merged extension brings the same lnb' into q's stay; q keeps its own state and
 * sum.  Selection order and tie rule are unchanged.  After frame n-1 with use_eos: total += alpha * final[state] (clamped at
 * -1e30), lmsum += final[state], and the live entries are re-ranked by the new total, ties by the previous rank.  n == 0 returns
 * the empty labelling with score alpha * final[start] (0 without use_eos).  The score of a result is
 *   ln(sum over its paths of P_ac) + alpha * ln P_lm(labels [, </s>]) + beta * |labels|.
 * Outputs as eesen_ctc_decode_parallel; lm_score_host [S][nbest] (may be NULL): each entry's lmsum, -1e30 beyond the returned
 * count (NaN under a raised guard word).  EESEN_ERR_INVALID besides that call's limits: lm == NULL, an LM built for another K,
 * use_eos on an LM without </s>, a non-finite lm_weight or insertion_bonus.  eesen_ctc_get_decode_times (the LM lookups are part
 * of the beam phase) and eesen_ctc_get_decode_candidates work after either call. */
int eesen_ctc_decode_parallel_lm(eesen_ctc_t* ctc, const int* frame_num_utt, int S, const float* scores_dev, int rows, int K, int ld,
                                 int is_log, int beam, int max_classes, int nbest, eesen_lm_t* lm, float lm_weight,
                                 float insertion_bonus, int use_eos, int* hyp_host /*S*nbest*T*/, int* hyp_len_host /*S*nbest*/,
                                 float* score_host /*S*nbest*/, float* lm_score_host /*S*nbest or NULL*/);

/* eesen_lm_create_from_arpa with skip_oov != 0: an n-gram that holds a word which is neither in the table nor <s>, </s>, <unk>
 * is dropped instead of being an error (the recipes' remove_oovs.pl before G is built).  Each section's count is checked against
 * the header with the dropped lines included.  skip_oov == 0 is eesen_lm_create_from_arpa.  eesen_lm_oov_dropped: how many
 * n-grams were dropped. */
int eesen_lm_create_from_arpa_ex(const char* arpa_path, const char* units_path /*or NULL*/, int K, int skip_oov, eesen_lm_t** lm);
int eesen_lm_oov_dropped(eesen_lm_t* lm, long long* ngrams);

/* ---- lexicon-constrained decoding (INTEGRATION.md "Lexicon"; no counterpart: the reference walks a TLG graph) ----
 * For systems whose words are sequences of units separated by one space unit (the recipes' character systems).  The lexicon file
 * holds one `word unit unit ...` line per spelling; units resolve through units_path (`symbol id`) or, with NULL, are decimal class
 * ids (the recipes' lexicon_numbers.txt).  A spelling is a non-empty sequence of classes in [1, K) other than space_class.  Word ids
 * are 1 .. V in order of first appearance; a word may have several spellings and may be a prefix of another; an identical line given
 * twice is accepted.  EESEN_ERR_INVALID with the file and the line: an unknown unit, a unit equal to space_class or outside [1, K),
 * an empty spelling, the same spelling for two words (both are named), a file without a word.
 * The trie: node 0 is the root, a node's children are sorted by class id, eesen_lex_word gives the word that ends at a node or 0,
 * eesen_lex_child the child for a class or -1.  eesen_lex_write_words writes `word id` lines: the table eesen_lm_create_from_arpa
 * takes as units_path, with K = V + 1, for a word LM.  eesen_lex_words segments a labelling of
 *   L = { empty } + { w1 Sp w2 Sp ... wn }     (exactly one space between words, none leading or trailing)
 * into words_out (room for (n + 1) / 2) and is EESEN_ERR_INVALID for a labelling outside L.  No device work here. */
int eesen_lex_create(const char* lexicon_path, const char* units_path /*or NULL*/, int K, int space_class, eesen_lex_t** lex);
int eesen_lex_destroy(eesen_lex_t* lex);
int eesen_lex_info(eesen_lex_t* lex, int* words, int* nodes, int* max_word_len);   /* any pointer may be NULL */
int eesen_lex_write_words(eesen_lex_t* lex, const char* path);
int eesen_lex_child(eesen_lex_t* lex, int node, int c, int* child);
int eesen_lex_word(eesen_lex_t* lex, int node, int* word);
int eesen_lex_words(eesen_lex_t* lex, const int* labels, int n, int* words_out, int* num_words);
/* eesen_ctc_decode_parallel restricted to L, with an optional LM over the word ids (lm: built with K = V + 1, or NULL).  An entry
 * also carries its lexicon node v, an LM state and lmsum (the empty prefix: 0, the start state, 0).  The extension p + c:
 *   c != Sp: allowed iff v has a child v' for c; the entry moves to v', LM state and lmsum stay, g = 0;
 *   c == Sp: allowed iff w = word[v] != 0; (wt, next) = lm_step(state, w) (0 and no state without an LM), g = lm_weight * wt +
 *            word_bonus, the entry moves to node 0, state next, lmsum + wt;
 * lnb' = (s_t(c) + g) + (c == e ? lb : tot) as in eesen_ctc_decode_parallel_lm; a disallowed extension is no candidate.  After
 * frame n-1 an entry is complete if it is empty or word[v] != 0; a non-empty complete one closes its last word (total += lm_weight
 * * wt + word_bonus, then with use_eos lm_weight * final[next]; lmsum takes the same terms unweighted), the empty one takes only
 * lm_weight * final[start] with use_eos; incomplete entries are dropped and the rest re-ranked, ties by previous rank.  An
 * utterance without a complete entry returns count 0 (all lengths -1, scores -1e30).  The score of a result is
 *   ln(sum over its paths of P_ac) + lm_weight * ln P_lm(words [, </s>]) + word_bonus * |words|.
 * Outputs as eesen_ctc_decode_parallel_lm; word_host [S][nbest][T] / word_len_host [S][nbest] (either may be NULL): the word ids of
 * each returned labelling, -1 beyond their number (and for absent entries).  EESEN_ERR_INVALID besides that call's limits:
 * lex == NULL, a lexicon built for another K, an LM whose K is not V + 1, use_eos without an LM or on one without </s>, a
 * non-finite lm_weight or word_bonus. */
int eesen_ctc_decode_parallel_lex(eesen_ctc_t* ctc, const int* frame_num_utt, int S, const float* scores_dev, int rows, int K, int ld,
                                  int is_log, int beam, int max_classes, int nbest, eesen_lex_t* lex, eesen_lm_t* lm /*or NULL*/,
                                  float lm_weight, float word_bonus, int use_eos, int* hyp_host /*S*nbest*T*/,
                                  int* hyp_len_host /*S*nbest*/, float* score_host /*S*nbest*/, float* lm_score_host /*S*nbest or NULL*/,
                                  int* word_host /*S*nbest*T or NULL*/, int* word_len_host /*S*nbest or NULL*/);

/* ---- words without a boundary unit (INTEGRATION.md "Words without a boundary unit": the recipes' phoneme systems) ----
 * The unspaced lexicon: the file format and the word ids of eesen_lex_create, but no boundary unit (nothing but CTC's blank sits
 * between words) and up to 15 words per spelling (homophones).  EESEN_ERR_INVALID with the file and the line: an unknown unit, a unit
 * outside [1, K), an empty spelling, a 16th word on one spelling (that line and the spelling's first are named), a file without a
 * word.  eesen_lex_max_homophones: H, the largest number of words on one spelling (0 for a lexicon of eesen_lex_create);
 * eesen_lex_node_words: the ascending word ids whose spelling ends at the node -- their number into *count, the first
 * min(count, cap) into out (out may be NULL with cap 0).  On an unspaced lexicon eesen_lex_word gives the smallest of them or 0 and
 * eesen_lex_words is EESEN_ERR_INVALID: a labelling does not determine its segmentation. */
int eesen_lex_create_unspaced(const char* lexicon_path, const char* units_path /*or NULL*/, int K, eesen_lex_t** lex);
int eesen_lex_max_homophones(eesen_lex_t* lex, int* H);
int eesen_lex_node_words(eesen_lex_t* lex, int node, int* out /*cap or NULL*/, int cap, int* count);
/* The word beam search along an unspaced lexicon (ctc_word_beam_kernel).  A hypothesis is a sequence of units and closing marks #w;
 * hypotheses with equal labels and different words are different entries and each carries the labels' full acoustic mass.  Entry p
 * at lexicon node v and candidate class c (e: p's last label) give, in this order,
 *   inside:  v has a child v' for c: p + c at v', g = 0, LM state and lmsum unchanged;
 *   close i: for the i-th word w of words(v), if the root has a child r for c: p + #w + c at r, (wt, next) = lm_step(state, w) (0
 *            without an LM), g = lm_weight * wt + word_bonus, state next, lmsum + wt;
 * lnb' = (s_t(c) + g) + (c == e ? lb : tot).  After frame n-1 a complete entry (empty, or words(v) non-empty) yields one result per
 * word of words(v), closed as in eesen_ctc_decode_parallel_lex; the results are ranked by total, ties by (previous rank, word
 * index).  Outputs as eesen_ctc_decode_parallel_lex, all from the device; word_end_host [S][nbest][T] (may be NULL): the number of
 * labels up to and including word j's last, -1 beyond the word count.  EESEN_ERR_INVALID besides that call's cases:
 * beam * (1 + max_classes * (1 + H)) above 4096 (the successor keys of a frame live in LDS), a lexicon of eesen_lex_create (that
 * one goes to eesen_ctc_decode_parallel_lex, which in turn refuses an unspaced lexicon). */
int eesen_ctc_decode_parallel_words(eesen_ctc_t* ctc, const int* frame_num_utt, int S, const float* scores_dev, int rows, int K, int ld,
                                    int is_log, int beam, int max_classes, int nbest, eesen_lex_t* lex, eesen_lm_t* lm /*or NULL*/,
                                    float lm_weight, float word_bonus, int use_eos, int* hyp_host /*S*nbest*T*/,
                                    int* hyp_len_host /*S*nbest*/, float* score_host /*S*nbest*/, float* lm_score_host /*S*nbest or NULL*/,
                                    int* word_host /*S*nbest*T or NULL*/, int* word_len_host /*S*nbest or NULL*/,
                                    int* word_end_host /*S*nbest*T or NULL*/);

/* ---- unigram LM look-ahead in the two lexicon searches (INTEGRATION.md "LM look-ahead") --------------------------------------------
 * The LM's weight joins a score only when a word closes; with the look-ahead on, a frame's candidates are RANKED as if the best
 * word still reachable had been paid already, so a narrow beam keeps the hypotheses inside frequent words.
 *   u(w)  = the weight eesen_lm_step(lm, 0, w) returns: ln P(w) in fp32, or <unk>'s where the file has no unigram for w;
 *   la[v] = max { u(w) : a spelling of w passes through or ends at lexicon node v } (comparisons only; la[0]: over the vocabulary).
 * eesen_lex_lookahead writes la into out_host [nodes] (eesen_lex_info); no device work.  EESEN_ERR_INVALID: an LM whose K is not
 * V + 1, cap < nodes.
 * eesen_ctc_set_lm_lookahead(ctc, mode): 0 = off (the default), 1 = unigram; any other value is EESEN_ERR_INVALID.  With mode 1
 * eesen_ctc_decode_parallel_lex and eesen_ctc_decode_parallel_words select a frame's best `beam` candidates by
 *   (total + eta) + 0,  eta = lm_weight * la[v] + word_bonus  (fp32; the sum clamped at -1e30 like every score)
 * in place of total, v the lexicon node the candidate stands on after the step (a stay: the entry's; a unit / an inside successor:
 * the child; a space: the root; a closing successor: the root's child for the class).  A candidate is dead by its real total; the
 * tie index, every carried value, the end of the utterance and the final ranking by the real total are unchanged, and a returned
 * score keeps its meaning.  The look-ahead is context-independent: one table per (lexicon, LM) pair, uploaded when the pair changes.
 * With the mode set, either call without a word LM is EESEN_ERR_INVALID; eesen_ctc_decode_parallel and _lm ignore the mode. */
int eesen_lex_lookahead(eesen_lex_t* lex, eesen_lm_t* lm, float* out_host /*cap*/, int cap);
int eesen_ctc_set_lm_lookahead(eesen_ctc_t* ctc, int mode);
int eesen_ctc_get_lm_lookahead(eesen_ctc_t* ctc, int* mode);

/* ---- time stamps and confidences of decoded hypotheses (INTEGRATION.md "Time stamps and CTM") --------------------------------------
 * Aligns every entry the LAST decode call on this Ctc returned (any of the four calls above) to the frames and says when each label
 * and each word was spoken and how sure the N-best list is of the word.  frame_num_utt, S, scores_dev, rows, K, ld, is_log: that
 * call's.  Each entry's labels are aligned on the acoustic scores alone by eesen_ctc_align_parallel's recurrence and tie rule (no LM
 * term, no bonus: they do not depend on the frame) -- all S * nbest lattices in one sweep launch and one traceback launch per group
 * of lattices (the delta rows of a group stay within 1 GiB), lattice i on the score rows of utterance i / nbest.
 *   lstart_host / lend_host [S][nbest][T] int32: first frame of label u on the path and one past its last; blank frames belong to
 *     no label; -1 beyond the labels.
 *   words: a run of labels [a, b] -- every label by itself with its class as the id (plain, token LM), the runs between the spaces
 *     with eesen_lex_words' ids (spaced lexicon; the space's frames belong to no word), the runs word_end_host gave (unspaced
 *     lexicon).  wstart_host / wend_host [S][nbest][T] int32 = lstart[a], lend[b]: blanks inside a word are inside its interval.
 *   wconf_host [S][nbest][T] float: eesen_word_confidence over the utterance's returned entries and their totals (score_host).
 *   path_score_host [S][nbest]: the best path's log-score.
 * Any output pointer may be NULL.  Conventions: the empty hypothesis has no lattice and no words, path score 0; an entry of more than
 * 2047 labels (L' > 4096) has path score -1e30 and -1 stamps (its words: empty intervals, confidence 0); ranks beyond the returned
 * count have -1 stamps, path score -1e30 and confidence -1e30, as have the slots beyond an entry's labels / words.  Under a raised
 * guard word (in the decode call or in this one): every stamp -1, path scores and confidences NaN.
 * EESEN_ERR_STATE: no decode call yet, or S, rows or frame_num_utt differ from the last decode call's.  EESEN_ERR_INVALID: ld < K, a
 * non-finite or negative conf_scale.  The lattice buffers are borrowed as by eesen_ctc_align_parallel.  The call waits for its results. */
int eesen_ctc_decode_stamps(eesen_ctc_t* ctc, const int* frame_num_utt, int S, const float* scores_dev, int rows, int K, int ld, int is_log,
                            double conf_scale, int* lstart_host /*S*nbest*T or NULL*/, int* lend_host /*S*nbest*T or NULL*/,
                            int* wstart_host /*S*nbest*T or NULL*/, int* wend_host /*S*nbest*T or NULL*/, float* wconf_host /*S*nbest*T or NULL*/,
                            float* path_score_host /*S*nbest or NULL*/);
/* seconds of the last eesen_ctc_decode_stamps' device work: out[0]=lattice build (with the logarithm when is_log == 0), [1]=max-plus
 * sweeps and tracebacks of all groups, [2]=stamps; summed over all calls since the last read under eesen_ctc_set_profiling(ctc, 2). */
int eesen_ctc_get_stamp_times(eesen_ctc_t* ctc, float* out3);
/* Test hook: sweep the lattices of eesen_ctc_decode_stamps in groups of `lattices` (0 = automatic: as many as 1 GiB of delta rows hold). */
int eesen_ctc_set_stamp_group(eesen_ctc_t* ctc, int lattices);
/* ---- exact scores and second-pass rescoring (INTEGRATION.md "Rescoring") -----------------------------------------------------------
 * a = ln p(labels | x) = ln of the sum over all CTC paths that collapse to the labels, by the alpha recurrence of
 * eesen_ctc_eval_parallel on the log-scores of the decode calls (posteriors through the logarithm, or given with is_log; clamped from
 * below at -1e30; blank = class 0), closed on the LARGER of the two final cells: a = m + log(1 + exp(n - m)).  (eval_parallel's own
 * ln p closes on the final blank, as the reference does, and is wrong where that cell is unreachable or far below the last label's.)
 * The sweep keeps no row: every labelling of a call is one workgroup of one launch, and the only device output is one float each.
 * The empty labelling: a = sum_t s_t(0), 0 over no frames.  No path (too few frames, a zero on every path): a = -1e30; read a result
 * <= -1e29 as infeasible.
 *
 * eesen_ctc_score_parallel: any labellings per utterance.  Utterance s owns the labellings hyp_off[s] .. hyp_off[s + 1] (hyp_off[0] = 0,
 * NH = hyp_off[S]); labelling h the labels label_ids[label_off[h] .. label_off[h + 1]).  score_host [NH].  EESEN_ERR_INVALID: a label
 * outside [1, K), ld < K, more than 2047 labels in a labelling, offsets that decrease.  Touches no statistic and nothing
 * eesen_ctc_get_alpha_beta reads.  NaN under a raised guard word.  The call waits for its results. */
int eesen_ctc_score_parallel(eesen_ctc_t* ctc, const int* frame_num_utt, int S, const float* scores_dev, int rows, int K, int ld, int is_log,
                             const int* hyp_off /*S+1*/, const int* label_off /*NH+1*/, const int* label_ids, float* score_host /*NH*/);
/* eesen_ctc_decode_rescore: the entries the LAST decode call on this Ctc returned (any of the four), scored exactly and ranked again.
 * frame_num_utt, S, scores_dev, rows, K, ld, is_log: that call's.  For entry i of an utterance:
 *   g_i = eesen_lm_score(lm, tokens_i, use_eos) in fp64 -- the tokens are the labels (plain, token LM; lm's K = K) or the word ids
 *         (both lexicon modes; lm's K = V + 1); with lm == NULL the first pass's LM sum (0 if that call had no LM);
 *   n_i = the number of tokens;   total_i = (float)((double)a_i + (double)lm_weight * g_i + (double)bonus * n_i).
 * am_score_host / lm_score_host / total_host [S][nbest] float, order_host [S][nbest] int32: the first-pass ranks by total descending,
 * ties to the smaller rank, then -- in rank order -- the infeasible entries (a <= -1e29, more than 2047 labels) and the ranks beyond
 * the returned count, all of which read -1e30 in the three score arrays.  Any output pointer may be NULL.  Under a raised guard word
 * (in the decode call or in this one): NaN scores, order -1.  Nothing the decode call left is changed: eesen_ctc_decode_stamps
 * afterwards is indexed by first-pass rank as before.
 * EESEN_ERR_STATE: no decode call yet, or S, rows or frame_num_utt differ from its.  EESEN_ERR_INVALID: ld < K, a non-finite lm_weight
 * or bonus, use_eos on an LM without </s>, an LM whose class count does not fit the mode.  The call waits for its results. */
int eesen_ctc_decode_rescore(eesen_ctc_t* ctc, const int* frame_num_utt, int S, const float* scores_dev, int rows, int K, int ld, int is_log,
                             eesen_lm_t* lm /*or NULL*/, float lm_weight, float bonus, int use_eos, float* am_score_host /*S*nbest or NULL*/,
                             float* lm_score_host /*S*nbest or NULL*/, float* total_host /*S*nbest or NULL*/, int* order_host /*S*nbest or NULL*/);
/* seconds of the last of the two calls above: out[0]=lattice build (with the logarithm when is_log == 0), [1]=the scoring sweep (both
 * device time), [2]=the host's LM scoring and ranking (0 after eesen_ctc_score_parallel). */
int eesen_ctc_get_rescore_times(eesen_ctc_t* ctc, float* out3);
/* ---- edit distances on the device and minimum Bayes risk over N-best lists (INTEGRATION.md "Minimum Bayes risk") --------------------
 * d(a, b) = the Levenshtein distance of two int32 token sequences, unit costs, the total only: what eesen_edit_distance returns, and
 * every integer equal to it.  One wavefront per pair, all pairs of a call in one launch (edit_distance_kernel).  At most 8192 tokens
 * per sequence.
 *
 * eesen_edit_distance_parallel: G groups of sequences.  Group g owns the sequences seq_off[g] .. seq_off[g + 1] (seq_off[0] = 0,
 * NQ = seq_off[G], n_g its count); sequence q the tokens tok_ids[tok_off[q] .. tok_off[q + 1]), any int32.  pair_host receives
 * n_g x n_g int32 per group, packed group after group: d of every two sequences of the group, 0 on the diagonal (the pairs i < j are
 * computed and mirrored).  With ref_off / ref_ids (group g's reference: ref_ids[ref_off[g] .. ref_off[g + 1]), may be empty)
 * ref_dist_host [NQ] receives every sequence's distance to its group's reference.  pair_host may be NULL; ref_off, ref_ids and
 * ref_dist_host are NULL together.  G = 0 and groups without a sequence are allowed.  EESEN_ERR_INVALID, before any launch: offsets
 * that decrease, a sequence or reference of more than 8192 tokens.  Touches no statistic and no buffer another call reads
 * afterwards.  The call waits for its results. */
int eesen_edit_distance_parallel(eesen_ctc_t* ctc, int G, const int* seq_off /*G+1*/, const int* tok_off /*NQ+1*/, const int* tok_ids,
                                 const int* ref_off /*G+1 or NULL*/, const int* ref_ids /*or NULL*/, int* pair_host /*sum n_g^2 or NULL*/,
                                 int* ref_dist_host /*NQ or NULL*/);
/* eesen_ctc_decode_mbr: N-best minimum Bayes risk (Stolcke et al. 1997) over the entries the LAST decode call on this Ctc returned (any
 * of the four), taken from where that call left them -- no labels travel through the caller.  S: that call's.
 *   level 0: an entry's tokens are the mode's LM tokens -- its labels (plain, token LM) or its word ids (both lexicon modes), the
 *            tokens eesen_ctc_decode_rescore scores;   level 1: always its labels (under a lexicon the space is a label like any other).
 *   z_i = total_host[s * nbest + i] if total_host is given (eesen_ctc_decode_rescore's totals), else the decode call's score.
 *   Entry i COUNTS if it is within the returned count, z_i > -1e29, z_i is not NaN and it has no more than 8192 tokens.
 * With c = scale (finite, >= 0), in fp64, every sum over the counting k in ascending rank:
 *   P_i = exp(c (z_i - z_max)) / sum_k exp(c (z_k - z_max));   risk_i = sum_k P_k d(i, k).
 * dist_host [S][nbest][nbest] int32: d(i, k), -1 where either entry does not count.  ref_dist_host [S][nbest] int32: d(i, reference of
 * utterance s) with ref_ids[ref_off[s] .. ref_off[s + 1]) the reference in the level's tokens; -1 where the entry does not count, and
 * everywhere without ref_off.  post_host / risk_host [S][nbest] double, -1e30 where the entry does not count.  order_host [S][nbest]
 * int32: the counting ranks by risk ascending, ties to the larger z, then to the smaller rank; then the others in rank order.
 * Any output may be NULL; when only ref_dist_host (or post_host) is asked for, the pairwise jobs are not launched.  Under a raised guard
 * word (in the decode call or in this one): dist, ref_dist and order -1, post and risk NaN.  Nothing the decode call left is changed:
 * eesen_ctc_decode_stamps and eesen_ctc_decode_rescore afterwards behave as before.
 * EESEN_ERR_STATE: no decode call yet, or S differs from its.  EESEN_ERR_INVALID: a non-finite or negative scale, a level outside
 * {0, 1}, reference offsets that decrease, a reference of more than 8192 tokens.  The call waits for its results. */
int eesen_ctc_decode_mbr(eesen_ctc_t* ctc, int S, int level, double scale, const float* total_host /*S*nbest or NULL*/,
                         const int* ref_off /*S+1 or NULL*/, const int* ref_ids /*or NULL*/, int* dist_host /*S*nbest*nbest or NULL*/,
                         int* ref_dist_host /*S*nbest or NULL*/, double* post_host /*S*nbest or NULL*/, double* risk_host /*S*nbest or NULL*/,
                         int* order_host /*S*nbest or NULL*/);
/* seconds of the last of the two calls above (all 0 before the first): out[0]=job build and uploads (host), [1]=the distance kernel
 * (device time), [2]=the host's mirroring, posteriors, risks and ranking.  Under eesen_ctc_set_profiling(ctc, 2) the three are summed
 * over the calls since they were last read. */
int eesen_ctc_get_mbr_times(eesen_ctc_t* ctc, float* out3);

/* N-best posterior word confidences in fp64 on the host; no device work.  Entry i of n_entries has the total scores[i] and word_len[i]
 * words (< 0: not an entry, skipped) with ids word_ids[i*stride + j] and frame intervals [wstart, wend).  With c = conf_scale (finite,
 * >= 0): P_i = exp(c (z_i - z_max)) / sum_k exp(c (z_k - z_max)) over the entries, and
 *   conf_out[i*stride + j] = sum_k P_k [entry k has a word of the same id whose interval intersects word j's]
 * -- each entry counts at most once; -1e30 beyond an entry's words.  One entry gives 1 everywhere. */
int eesen_word_confidence(int n_entries, const double* scores, const int* word_len, const int* word_ids, const int* wstart, const int* wend,
                          int stride, double conf_scale, double* conf_out /*n_entries*stride*/);

/* LevenshteinEditDistance (src/util/edit-distance-inl.h), total errors only: the count eesen_ctc_error_rate_mseq accumulates, for a
 * host that scores hypotheses of its own (ctc-decode --ref-rspecifier).  No device work. */
int eesen_edit_distance(const int* ref, int num_ref, const int* hyp, int num_hyp, int* errors);

/* ---- CE (src/net/ce-loss.h:32-77): frame-level cross-entropy ----------------------------------- */
int eesen_ce_create(int device, void* stream, eesen_ce_t** out);
int eesen_ce_destroy(eesen_ce_t* ce);
/* CE::EvalParallel (src/net/ce-loss.cc:94-169) in ONE pass over the posteriors.  net_out_dev: [T*S x K] softmax outputs
 * (device, row t*S + s, leading dimension ld), frame_num_utt: host int[S]; row t*S + s is valid iff t < frame_num_utt[s] (the
 * trainer's frame_mask_host, train-ce-parallel.cc:176-184).  targets_host: int[rows], one class id per row; only the valid
 * rows' ids are read, and each must lie in [0, K) (EESEN_ERR_INVALID with the reference's message otherwise).  Writes diff_dev
 * [T*S x K] (device, diff_ld) = (y - onehot(target)) on valid rows and 0 on padded rows: d(CE)/d(logits), which the Net's
 * <Softmax> passes through unchanged.  Accumulates, in call order: obj += sum over valid rows of -ln y[target], correct +=
 * valid rows whose first argmax is the target, frames += rows (PADDED rows, as the reference counts), sequences += S, and the
 * progressive report of ce-loss.cc:153-167 (eesen_ce_progress).  obj_host (may be NULL: then nothing waits for the device and
 * the sums join the totals when they have arrived): this call's objective.  Statistics are reduced in a fixed order: the same
 * inputs give the same bits on every run.  CE::Eval (:30-92) is this call with S = 1 and frame_num_utt[0] = rows. */
int eesen_ce_eval_parallel(eesen_ce_t* ce, const int* frame_num_utt, int S, const float* net_out_dev, int rows, int K, int ld,
                           const int* targets_host, float* diff_dev, int diff_ld, double* obj_host);
/* CE::SetReportStep (ce-loss.h:47): a progress line is produced when the sequences since the last one EXCEED the step (100 until set) */
int eesen_ce_set_report_step(eesen_ce_t* ce, int report_step);
/* Running totals: obj (sum of -ln y[target]), correct frames, frames (padded rows), sequences.  Waits for pending calls. */
int eesen_ce_stats(eesen_ce_t* ce, double* obj, long* correct, long* frames, long* sequences);
/* CE::Report (ce-loss.cc:171-175): "\nFRAME_ACCURACY >> x% <<" with the TRUE ratio correct / frames (the reference divides two
 * int32 and prints 0 or 100).  NUL-terminated into buf[cap]; EESEN_ERR_INVALID when it does not fit. */
int eesen_ce_report(eesen_ce_t* ce, char* buf, int cap);
/* The progress lines of ce-loss.cc:153-167 (the reference's KALDI_LOG text, byte for byte), one per call, oldest first; "" when
 * none is ready.  A line is ready once the sums of the call that produced it have arrived: wait != 0 waits for every pending
 * call first, wait == 0 never blocks (a line then appears up to two calls late, with the same text). */
int eesen_ce_progress(eesen_ce_t* ce, int wait, char* buf, int cap);
/* As eesen_ctc_set_guard: a minibatch computed while the Net's recurrence error word was set is dropped from every total
 * (eesen_ce_dropped counts them) and its obj_host reads NaN.  net == NULL removes the guard. */
int eesen_ce_set_guard(eesen_ce_t* ce, eesen_net_t* net);
int eesen_ce_dropped(eesen_ce_t* ce, long* minibatches);
/* seconds of the last eval's device work (the fused pass + its fixed-order reduction); mode 2 sums all calls since the last read */
int eesen_ce_set_profiling(eesen_ce_t* ce, int mode);
int eesen_ce_get_phase_times(eesen_ce_t* ce, float* out1);

/* ---- dropout variants of BiLstm(Parallel) (src/net/bilstm-parallel-layer.h:46-94,209-377,604-879) ------
 * Options travel in the model file (nine tokens, src/net/bilstm-layer.h:331-373) and through set/get_layer_dropout, in token
 * order: {ForwardDropoutFactor, ForwardTimeStepDropout, ForwardSequenceDropout, RecurrentTimeStepDropout,
 * RecurrentSequenceDropout, RNNDrop, NoMemLossDropout, RecurrentDropoutFactor, TwiddleForward} (booleans as 0 / 1).
 * Net::SetTrainMode / SetTestMode (src/net/net.cc:396-412): dropout is applied in train mode only (the default).
 * Masks (values 0 or 1/(1-p)) are drawn on the device from (seed, draw counter, element) -- the reference draws them with the
 * host RNG and copies them over (:50-62).  For parity tests the masks of the NEXT eesen_net_propagate can be supplied:
 *   fwd_mask  [T*S x 2H] or NULL;  rec_mask [rec_rows x 2H] with rec_rows = (T+2)*S (time-step masks, row t*S+s as in the
 *   reference's buffers) or S (sequence masks), columns = forward-direction H then backward-direction H, or NULL;
 *   twiddle_coin: 0 / 1 = value of the TwiddleForward coin, -1 = draw it.
 * H is the cell count per direction of the MODEL FILE's layer (eesen_net_layer_info's output dimension / ndir): when the library
 * pads a cell count that is not a multiple of 4 inside, these two accessors gather / scatter the file's columns. */
int eesen_net_set_train_mode(eesen_net_t* net, int train);
int eesen_net_set_dropout_seed(eesen_net_t* net, unsigned long long seed);
int eesen_net_set_layer_dropout(eesen_net_t* net, int layer, const float* nine);
int eesen_net_get_layer_dropout(eesen_net_t* net, int layer, float* nine);
int eesen_net_set_dropout_masks(eesen_net_t* net, int layer, const float* fwd_mask_host, long fwd_floats,
                                const float* rec_mask_host, int rec_rows, long rec_floats, int twiddle_coin);
/* masks used by the LAST propagate: fwd_mask_host [T*S x 2H], rec_mask_host [(T+2)*S x 2H] (either may be NULL);
 * info4 = {forward dropout applied, recurrent mode (0 none, 1 no-memory-loss, 2 RNNDrop), twiddle coin, 2H}. */
int eesen_net_get_dropout_masks(eesen_net_t* net, int layer, float* fwd_mask_host, float* rec_mask_host, int* info4);

/* ---- minibatch assembly on the device (row a1) ---------------------------------------------------
 * Replaces the host-side padding + interleave + blocking H2D of src/netbin/train-ctc-parallel.cc:186-195: the S utterance
 * matrices are packed back to back into a pinned staging slot (no padding crosses PCIe), copied on the feeder's own
 * stream, and a kernel writes the zero-padded time-major matrix (row t*S + s, leading dimension ld = D rounded up to 4)
 * in HBM.  `slots` staging slots rotate: submit() of batch n+1 overlaps the training step of batch n.
 *   submit : host pointers utts[s] -> [frames[s] x D] row-major, row stride strides[s] floats (strides == NULL: D).
 *            Asynchronous; blocks only if the slot being reused is still in flight / not yet released.
 *   acquire: makes `compute_stream` wait (on the device) for the slot; returns the assembled device matrix.  The
 *            pointer stays valid until the slot is submitted again.
 *   release: call after the last consumer of the slot has been ENQUEUED on compute_stream (eesen_net_propagate copies
 *            its input, so right after it). */
typedef struct eesen_feeder eesen_feeder_t;
int eesen_feeder_create(int device, void* compute_stream, int slots, eesen_feeder_t** out);
int eesen_feeder_destroy(eesen_feeder_t* f);
int eesen_feeder_submit(eesen_feeder_t* f, const float* const* utts, const int* frames, const int* strides, int S, int D,
                        int* slot);
int eesen_feeder_acquire(eesen_feeder_t* f, int slot, float** feats_dev, int* T, int* S, int* ld);
int eesen_feeder_release(eesen_feeder_t* f, int slot);

/* ---- feature front end fused into the batch assembly (the step in front of the path) --------
 * The recipes hand the trainer its features through a pipe of host filters (asr_egs/wsj/steps/train_ctc_parallel.sh:95-110,
 * decode_ctc_lat.sh:92-95, librispeech/steps/train_ctc_parallel_mult.sh:110-133):
 *   apply-cmvn [--norm-vars] --utt2spk=... scp:cmvn.scp scp:train.scp ark:- | splice-feats --left-context=L --right-context=R
 *   ark:- ark:- | subsample-feats --n=N --offset=O ark:- ark:- | add-deltas ark:- ark:- |
 * With a pipeline set, submit_raw takes the RAW utterance matrices (what scp:train.scp points at) and the stages run on
 * the device, in the given order, between the PCIe copy and the interleave; acquire() then returns [T*S x D_out] with
 * T = the longest utterance AFTER the pipeline.  Stage arithmetic is the reference tool's, operation for operation:
 *   EESEN_FEAT_CMVN       src/featbin/apply-cmvn.cc, ApplyCmvn src/feat/cmvn.cc:110-117: x * scale[d] + offset[d]; the two
 *                         vectors per utterance come with submit_raw (eesen_cmvn_norm computes them from the stats matrix)
 *   EESEN_FEAT_SPLICE     src/featbin/splice-feats.cc, SpliceFrames src/feat/feature-functions.cc:391-412; a = left, b = right
 *   EESEN_FEAT_SUBSAMPLE  src/featbin/subsample-feats.cc:77-108; a = n (n < 0: repeat every frame -n times), b = offset
 *   EESEN_FEAT_DELTAS     src/featbin/add-deltas.cc, DeltaFeatures src/feat/feature-functions.cc:210-267; a = order, b = window
 * An utterance that the pipeline leaves without frames (subsampling offset beyond its end) contributes no rows, like the
 * reference tool, which writes no output for it; the caller drops it from the labels (eesen_feeder_pipeline_shape tells). */
#define EESEN_FEAT_CMVN 1
#define EESEN_FEAT_SPLICE 2
#define EESEN_FEAT_SUBSAMPLE 3
#define EESEN_FEAT_DELTAS 4
/* compute-fbank-feats in front of the filters (see "log-mel filterbank features" below): legal only as stage 0, configured beforehand by
 * eesen_feeder_set_fbank; a and b are unused.  submit_raw then takes waveforms as [samples x 1] matrices (D_in = 1, frames[s] = the
 * sample count), eesen_feeder_pipeline_shape(f, 1, nsamp, ...) answers through it, and the CMVN vectors have the filterbank dimension.
 * The kernel writes straight into the packed buffer the next stage reads.  Every waveform submitted gets a fresh dither key (a counter
 * per feeder), so an epoch's noise differs from the last one's while a feeder fed the same sequence reproduces its batches. */
#define EESEN_FEAT_FBANK 5
/* paste-feats --length-tolerance=a "compute-fbank-feats ..." "compute-kaldi-pitch-feats ... | process-kaldi-pitch-feats ..." in front of
 * the filters (the tonal recipes' features, asr_egs/wsj/steps/make_fbank_pitch.sh:117-121; INTEGRATION.md "Fbank + pitch"): legal only
 * as stage 0, configured beforehand by eesen_feeder_set_fbank AND eesen_feeder_set_pitch, whose samp_freq must agree; a = the length
 * tolerance (>= 0), b is unused.  Input as for EESEN_FEAT_FBANK ([samples x 1], D_in = 1).  The samples go up once; the filterbank,
 * the four pitch launches (post-processing included) and the join run back to back on the feeder's stream.  Output columns: the
 * filterbank's, then the processed pitch's.  Rows: eesen_feat_paste_frames of the filterbank's frame count and the processed pitch
 * matrix's row count (frames + delay, 0 without a frame) -- an utterance it leaves without rows is dropped as above.  A waveform's
 * key (the feeder's counter) is the same for the dither and for the delta-pitch noise.  A batch beyond 2^30 filterbank frames or 2^28
 * pitch frames is EESEN_ERR_INVALID. */
#define EESEN_FEAT_FBANK_PITCH 6
typedef struct eesen_feat_stage { int kind, a, b; } eesen_feat_stage_t;
int eesen_feeder_set_pipeline(eesen_feeder_t* f, const eesen_feat_stage_t* stages, int n_stages); /* 0 stages: plain submit */
struct eesen_fbank_opts;
int eesen_feeder_set_fbank(eesen_feeder_t* f, const struct eesen_fbank_opts* opts);   /* before a pipeline that starts with EESEN_FEAT_FBANK */
struct eesen_pitch_opts;
int eesen_feeder_set_pitch(eesen_feeder_t* f, const struct eesen_pitch_opts* opts);   /* and before one that starts with EESEN_FEAT_FBANK_PITCH; carries eesen_pitch_create's refusals */
/* AppendFeats' length rule (src/featbin/paste-feats.cc:35-56) on the row counts of one utterance in n_inputs (>= 1) tables, host only:
 * *out <- the shortest count, or 0 (the utterance is dropped) when the longest exceeds it by more than tolerance or an input is empty */
int eesen_feat_paste_frames(const int* frames, int n_inputs, int tolerance, int* out);
/* paste-feats for callers that hold tables: inputs[j][s] -> host matrix [frames[j * S + s] x dims[j]] row-major of input j (2..4
 * inputs), out[s] -> host room for [rows x sum of dims] (may be NULL for a dropped utterance), frames_out[s] (may be NULL) <- rows by the
 * rule above.  One upload, the feeder's join kernel, one copy back on `stream`.  Synchronises. */
int eesen_paste_feats(int device, void* stream, const float* const* const* inputs, const int* dims, int n_inputs, const int* frames,
                      int S, int tolerance, float* const* out, int* frames_out);
/* feature dimension / frame count behind the pipeline for an utterance of [frames_in x D_in] (either output may be NULL) */
int eesen_feeder_pipeline_shape(eesen_feeder_t* f, int D_in, int frames_in, int* D_out, int* frames_out);
/* cmvn[s] -> 2 x Dc floats (offsets, then scales), Dc = the dimension in front of the CMVN stage; NULL without such a stage */
int eesen_feeder_submit_raw(eesen_feeder_t* f, const float* const* utts, const int* frames, const int* strides,
                            const float* const* cmvn, int S, int D_in, int* slot);
/* ApplyCmvn's normaliser (src/feat/cmvn.cc:78-108) on the host: stats = [rows x cols] doubles as apply-cmvn reads them
 * (row 0: sums and, last, the count; row 1: sums of squares), cols = dim + 1 -> offset_scale[2 x dim] */
int eesen_cmvn_norm(const double* stats, int rows, int cols, int norm_vars, float* offset_scale);

/* ---- CMVN statistics on the device (compute-cmvn-stats; INTEGRATION.md "CMVN statistics") -----------------------
 * Per utterance the [2 x (D+1)] double matrix apply-cmvn reads: row 0 the sums of x * w and, last, the count (the sum of w); row 1
 * the sums of (x * x) * w and a 0.  As in the reference the products are FLOAT products, rounded to fp32 before they are widened and
 * added in fp64, and a row whose weight is 0 is skipped (a row of infinities under weight 0 leaves the statistics finite).  Sums are
 * fp64 from the first add, combined in a fixed order without atomics: an utterance's statistics are the same bits in every call,
 * whatever stands beside it in the batch. */
/* AccCmvnStats (src/feat/cmvn.cc:30-62) for a minibatch of matrices on the host: utts[s] -> [frames[s] x D] with row stride
 * strides[s] (NULL: D); weights NULL, or weights[s] NULL (all ones) or -> frames[s] floats; stats <- [S x 2 x (D+1)] doubles.
 * Synchronises. */
int eesen_cmvn_stats_parallel(int device, void* stream, const float* const* utts, const int* frames, const int* strides,
                              const float* const* weights, int S, int D, double* stats);
/* The same statistics of what the feeder's pipeline holds at stage boundary b (0: what was submitted, k: what stage k-1 wrote;
 * -1: off, the default), computed beside the batch assembly; unweighted.  Drains the feeder like the other set_* calls;
 * EESEN_ERR_INVALID for a boundary beyond the current pipeline, and eesen_feeder_set_pipeline refuses a pipeline that would leave
 * the tap beyond its last boundary. */
int eesen_feeder_set_stats_tap(eesen_feeder_t* f, int boundary);
/* stats <- [S x 2 x (D+1)] of the batch in `slot`, *D <- the dimension at the tapped boundary; waits for the slot's batch.
 * EESEN_ERR_STATE with the tap off, or for a batch submitted without it. */
int eesen_feeder_stats(eesen_feeder_t* f, int slot, double* stats, int* D);
/* average ms of `iters` back-to-back launches after one warm-up, without the copies (as eesen_fbank_bench) */
int eesen_cmvn_stats_bench(int device, void* stream, const float* const* utts, const int* frames, int S, int D, int iters, float* avg_ms);

/* ---- log-mel filterbank features from waveforms (compute-fbank-feats; INTEGRATION.md "Fbank") ------------------
 * Fbank::ComputeInternal (src/feat/feature-fbank.cc:104-183) over a minibatch of ragged waveforms in ONE launch: per frame
 * ExtractWindow (src/feat/feature-functions.cc:91-167: cut [reflected without snip_edges], dither, DC removal, raw log
 * energy, pre-emphasis, window function, zero padding), a real FFT of N = 256 / 512 / 1024 / 2048 points, the power spectrum
 * of bins 0 .. N/2-1, the triangular mel filters of MelBanks (src/feat/mel-computations.cc:32-135) as a CSR table, floor at
 * FLT_MIN and log, and the optional energy column (first; last with htk_compat).  Samples are in int16 scale, as floats.
 * The struct carries the fields and defaults of FbankOptions, FrameExtractionOptions and MelBanksOptions.
 * Deviations: dither is a counter-based generator keyed by (dither_seed, utterance id, frame, sample) with Box-Muller, so a
 * seed reproduces its result (the reference draws from rand()); dither = 0 is the path held to the reference.  Refused with
 * EESEN_ERR_INVALID: round_to_power_of_two = 0, a padded window outside 256 .. 2048, htk_mode. */
#define EESEN_WINDOW_HAMMING 0
#define EESEN_WINDOW_HANNING 1
#define EESEN_WINDOW_POVEY 2
#define EESEN_WINDOW_RECTANGULAR 3
typedef struct eesen_fbank_opts {
  float samp_freq, frame_shift_ms, frame_length_ms, dither, preemph_coeff;           /* 16000, 10, 25, 1.0, 0.97 */
  int remove_dc_offset, window_type, round_to_power_of_two, snip_edges;              /* 1, POVEY, 1, 1 */
  int num_bins;                                                                      /* 23 */
  float low_freq, high_freq, vtln_low, vtln_high;                                    /* 20, 0, 100, -500 */
  int htk_mode;                                                                      /* 0 (refused otherwise) */
  int use_energy;                                                                    /* 0 */
  float energy_floor;                                                                /* 0 */
  int raw_energy, htk_compat, use_log_fbank;                                         /* 1, 0, 1 */
  float vtln_warp;                                                                   /* 1.0: one factor per extractor */
  unsigned long long dither_seed;                                                    /* 0 */
} eesen_fbank_opts_t;
typedef struct eesen_fbank eesen_fbank_t;
int eesen_fbank_opts_default(eesen_fbank_opts_t* opts);
/* create checks the options and builds the host tables; the device is first touched by eesen_fbank_compute (so shapes can be asked
 * for, and options refused, on a host without one) */
int eesen_fbank_create(int device, void* stream, const eesen_fbank_opts_t* opts, eesen_fbank_t** out);
int eesen_fbank_destroy(eesen_fbank_t* fb);
/* NumFrames (feature-functions.cc:29-48) in both edge modes, and num_bins + use_energy; either output may be NULL */
int eesen_fbank_shape(eesen_fbank_t* fb, int nsamp, int* frames, int* dim);
/* waves[s] -> nsamp[s] samples; utt_ids (NULL: 0 .. S-1) key the dither; out_host[s] -> [frames x dim] row-major (may be NULL
 * for an utterance without frames).  Synchronises. */
int eesen_fbank_compute(eesen_fbank_t* fb, const float* const* waves, const int* nsamp, const unsigned long long* utt_ids, int S,
                        float* const* out_host);
/* Average milliseconds (HIP events) of `iters` back-to-back launches of the kernel on these waveforms, after one warm-up launch and
 * without the copies; microbenchmark entry point used by scripts/fbank_probe.py. */
int eesen_fbank_bench(eesen_fbank_t* fb, const float* const* waves, const int* nsamp, int S, int iters, float* avg_ms);
/* The filter table of MelBanks for opts (vtln_warp included), host only: first[num_bins], size[num_bins], and the weights of all
 * bins back to back (*n_weights of them; written when weights != NULL and weights_cap suffices).  Carries the reference's
 * option checks: at least 3 bins, the frequency and VTLN ranges, "num-mel-bins too large". */
int eesen_fbank_mel_banks(const eesen_fbank_opts_t* opts, int* first, int* size, float* weights, int weights_cap, int* n_weights);

/* ---- Kaldi pitch features from waveforms (compute-kaldi-pitch-feats | process-kaldi-pitch-feats; INTEGRATION.md "Pitch") ------
 * The offline path of ComputeKaldiPitch (src/feat/pitch-functions.cc:1244-1280) and ProcessPitch (:1536-1549) over a minibatch of
 * ragged waveforms, four launches: the Hann-windowed-sinc down-sampler of LinearResample to resample_freq with the fp64 sums of the
 * signal, the NCCF of every frame on the integer lags with and without the ballast and its up-sampling to the geometric lag grid
 * (ArbitraryResample as a CSR table), the Viterbi search over the lag states with the energy re-estimate of RecomputeBacktraces at
 * its head and the traceback at its end, and the post-processing.  The search takes the exact minimum over all predecessor states,
 * ties to the lowest (the reference's pitch_use_naive_search branch); its arithmetic is float32 in a fixed order without fused
 * multiply-add (csrc/pitch.hip's header).  The struct carries the fields and defaults of PitchExtractionOptions and
 * ProcessPitchOptions.  Deviations: the delta-pitch noise is the fbank dither's counter-based generator keyed by (noise_seed,
 * utterance id, frame), so a seed reproduces (the reference draws RandGauss()); delta_pitch_noise_stddev = 0 is the path held to
 * the reference.  Refused with EESEN_ERR_INVALID: preemph_coeff != 0, frames_per_chunk != 0, simulate_first_pass_online,
 * nccf_ballast_online, resample_freq <= 2 * lowpass_cutoff, soft_min_f0 > min_f0, more than 1024 lag states, no output column.
 * max_frames_latency is accepted and has no effect offline, as in the reference. */
typedef struct eesen_pitch_opts {
  float samp_freq, frame_shift_ms, frame_length_ms, preemph_coeff;                    /* 16000, 10, 25, 0 (refused otherwise) */
  float min_f0, max_f0, soft_min_f0, penalty_factor;                                  /* 50, 400, 10, 0.1 */
  float lowpass_cutoff, resample_freq, delta_pitch, nccf_ballast;                     /* 1000, 4000, 0.005, 7000 */
  int lowpass_filter_width, upsample_filter_width;                                    /* 1, 5 */
  int max_frames_latency, frames_per_chunk, simulate_first_pass_online;               /* 0, 0 (refused otherwise), 0 (refused) */
  int recompute_frame, nccf_ballast_online, snip_edges;                               /* 500, 0 (refused otherwise), 1 */
  float pitch_scale, pov_scale, pov_offset, delta_pitch_scale, delta_pitch_noise_stddev;   /* 2, 2, 0, 10, 0.005 */
  int normalization_left_context, normalization_right_context, delta_window, delay;   /* 75, 75, 2, 0 */
  int add_pov_feature, add_normalized_log_pitch, add_delta_pitch, add_raw_log_pitch;  /* 1, 1, 1, 0 */
  unsigned long long noise_seed;                                                      /* 0 */
} eesen_pitch_opts_t;
typedef struct eesen_pitch eesen_pitch_t;
int eesen_pitch_opts_default(eesen_pitch_opts_t* opts);
/* create checks the options and builds the host tables (filter phases, lag grid, up-sampling CSR); the device is first touched by a
 * compute call, so shapes can be asked for, and options refused, on a host without one */
int eesen_pitch_create(int device, void* stream, const eesen_pitch_opts_t* opts, eesen_pitch_t** out);
int eesen_pitch_destroy(eesen_pitch_t* p);
/* frames of a waveform of nsamp samples (NumFramesAvailable after InputFinished, pitch-functions.cc:760-775; NOT the filterbank's
 * count), 2, and the number of selected post-processing columns; the processed matrix has frames + delay rows.  Outputs may be NULL */
int eesen_pitch_shape(eesen_pitch_t* p, int nsamp, int* frames, int* raw_dim, int* processed_dim);
/* waves[s] -> nsamp[s] samples in int16 scale; utt_ids (NULL: 0 .. S-1) key the noise.  process = 0: out[s] <- [frames x 2] (NCCF at
 * the chosen lag without ballast, pitch in Hz); process = 1: the post-processing runs on them in the same call, without a copy back in
 * between, and out[s] <- [frames + delay x processed_dim].  out_cap[s]: floats out[s] holds (NULL: trusted); out[s] may be NULL for a
 * waveform without a frame.  frames_out (may be NULL) <- rows written per waveform.  Synchronises. */
int eesen_pitch_compute(eesen_pitch_t* p, const float* const* waves, const int* nsamp, const unsigned long long* utt_ids, int S,
                        int process, float* const* out, const long* out_cap, int* frames_out);
/* the post-processing alone, for raw pairs that come from a table: raw[s] -> [frames[s] x 2] */
int eesen_pitch_process(eesen_pitch_t* p, const float* const* raw, const int* frames, const unsigned long long* utt_ids, int S,
                        float* const* out, const long* out_cap, int* frames_out);
/* DIAGNOSTIC: the stage outputs of one waveform, which the tests hold one by one.  counts[5] <- frames, frames of the first pass
 * (those that see window + last lag samples before the flush), lag states, down-sampled samples, of which before the flush.  Every
 * other output may be NULL and is sized by the caller from counts (ask once with NULLs): down [samples], nccf_pitch and nccf_pov
 * [frames x states] (up-sampled; nccf_pitch BEFORE the re-estimate's scaling), lags [states], avg_norm_prod [frames], mean_square
 * [2] (without and with the flushed tail), fwd [states] (forward costs after the last frame), backptr [frames x states], track
 * [frames], raw [frames x 2], taken <- whether the energy re-estimate was applied. */
int eesen_pitch_nccf(eesen_pitch_t* p, const float* wave, int nsamp, int* counts, float* down, float* nccf_pitch, float* nccf_pov,
                     float* lags, float* avg_norm_prod, double* mean_square, float* fwd, unsigned short* backptr, int* track,
                     float* raw, int* taken);
/* The lag grid of SelectLags (pitch-functions.cc:155-165) in seconds, host only: *n <- its size; written when lags != NULL and cap
 * suffices */
int eesen_pitch_lags(const eesen_pitch_opts_t* opts, float* lags, int cap, int* n);
/* Average milliseconds (HIP events) over `iters` repetitions of the launches on these waveforms, after one warm-up pass and without
 * the copies: avg_ms[5] <- all four launches back to back, then the down-sampler, the NCCF, the search and the post-processing
 * alone; microbenchmark entry point used by scripts/pitch_probe.py. */
int eesen_pitch_bench(eesen_pitch_t* p, const float* const* waves, const int* nsamp, int S, int iters, float* avg_ms);

/* ---- raw device helpers for hosts that own no GPU allocator --------------------------------- */
int eesen_dev_alloc(int device, long bytes, void** dev_ptr);
int eesen_dev_free(int device, void* dev_ptr);
int eesen_dev_copy(int device, void* dst, const void* src, long bytes, int kind /*1 H2D, 2 D2H, 3 D2D*/);

/* ---- single-op entry points (kernel-level parity tests and microbenchmarks) ------------------- */
/* C[MxN] = alpha*op(A)*op(B) + beta*C (+ bias[n]); fp32 MFMA GEMM on device pointers.
 * a_kc: A stored [M x K] (k contiguous) if 1, [K x M] if 0.  b_kc: B stored [N x K] if 1, [K x N] if 0.
 * Replaces CuMatrixBase::AddMatMat (src/gpucompute/cuda-matrix.cc:604-639). */
int eesen_op_gemm(int device, void* stream, int a_kc, int b_kc, int M, int N, int K, float alpha,
                  const float* A, int lda, const float* B, int ldb, float beta, float* C, int ldc,
                  const float* bias);

/* The same GEMM ENQUEUED on `stream` and nothing else (no allocation, no synchronisation): `ws` / `ws_floats` is the caller's split-K
 * workspace (device memory, 0 floats = no split-K), `extra_lds_bytes` the unused dynamic LDS that caps the kernel's workgroups per CU --
 * how Net::Backpropagate runs its weight-gradient GEMMs beside a recurrence (scripts/corun_probe.py measures what that costs either side). */
int eesen_op_gemm_async(int device, void* stream, int a_kc, int b_kc, int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                        float* C, int ldc, float* ws, long ws_floats, int extra_lds_bytes);

/* Post-processing of net-output-extract (src/netbin/net-output-extract.cc:103-112) on a device matrix, in place:
 * CuMatrixBase::ApplyLog when apply_log != 0, then ClassPrior::SubtractOnLogpost (src/net/class-prior.cc:80-91)
 * m[r][k] -= prior_scale * log_priors[k] when log_priors_host (cols floats) is not NULL.  Synchronises. */
int eesen_op_log_sub_prior(int device, void* stream, float* m_dev, int rows, int cols, int ld, int apply_log,
                           const float* log_priors_host, float prior_scale);

/* Average milliseconds (HIP events) of `iters` back-to-back launches of the same GEMM (beta = 0, no bias);
 * microbenchmark entry point used by scripts/gemm_bench.py. */
int eesen_op_gemm_bench(int device, int a_kc, int b_kc, int M, int N, int K, const float* A, int lda,
                        const float* B, int ldb, float* C, int ldc, int iters, float* avg_ms);

/* The operand bounds of the two-plane GEMM arithmetic (eesen_set_gemm_mode(2), csrc/gemm.hip: amax_rows_cols), as the Net measures
 * them: out_rows[r] = max_c |m[r][c]| (rows floats) and / or out_cols[c] = max_r |m[r][c]| (cols floats) of a device matrix with row
 * stride ld, in ONE pass; either output may be NULL.  Device pointers.  Synchronises.
 * No counterpart in the reference (its GEMM is cublasSgemm, src/gpucompute/cuda-matrix.cc:604-639): exported for the tests. */
int eesen_op_amax_rows_cols(int device, const float* m_dev, long rows, int cols, int ld, float* out_rows_dev, float* out_cols_dev);

#ifdef __cplusplus
}
#endif
#endif /* EESEN_HIP_H_ */
