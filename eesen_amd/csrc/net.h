// net.h -- host-side Net / Ctc objects behind the C-ABI (include/eesen_hip.h).
#pragma once
#include <string>
#include <vector>

#include "ctc_layout.h"
#include "kernels.h"
#include "lex.h"
#include "lm.h"
#include "tuning.h"

namespace eesen {

inline int pad4(int x) { return (x + 3) & ~3; }
constexpr size_t kCtlWords = 2 * kCtlHalf + 32;  // counters [0, kCtlHalf) forward, [kCtlHalf, 2 kCtlHalf) backward, last word = error flag

struct Layer {
  int kind = 0, din = 0, dout = 0;
  float coef = 1.f, max_grad = 0.f;
  // parameter block inside the net-wide flat buffers (library-internal layout)
  size_t p_off = 0, p_n = 0;
  // LSTM kinds
  int H = 0, ndir = 0;
  // FILE-side dimensions: what the model file, the Net::GetParams order and eesen_net_layer_info carry.  They differ from the internal
  // ones (din, dout, H -- what every kernel sees) only around an LSTM layer whose cell count per direction is not a multiple of 4:
  // the library pads such a layer with cells that are identically zero and stay so (zero rows, bias and peepholes; zero columns
  // wherever their output is read -- the argument and its test: eesen_amd/model_tools.py pad-cells, tests/test_gpu_parity.py), because
  // the kernels fetch the state four cells at a time.  Parameter I/O (for_each_param), the statistics and the model writer map
  // between the two; nothing else knows.
  int din_f = 0, dout_f = 0, Hf = 0;
  // where this layer's FILE input column d lives in its internal input: in_nb runs of in_hf columns, each at a stride of in_hi
  // (in_nb = 0: identity); out_*: the same for the columns this layer hands on
  int in_nb = 0, in_hf = 0, in_hi = 0, out_nb = 0, out_hf = 0, out_hi = 0;
  int in_col(int d) const { return in_nb ? (d / in_hf) * in_hi + d % in_hf : d; }
  size_t off_wx = 0, off_bias = 0, off_wm = 0, off_peep = 0;  // relative to p_off
  DevBuf<float> WmT;      // [ndir][H x 4H], rebuilt after every parameter change
  DevBuf<float> G, C, Y;  // activations
  DevBuf<float> X;        // exchange copy of Y in the persistent forward kernel's fetch order (LstmLayerDev::X)
  // AffineTransform
  size_t off_w = 0, off_b = 0;
  DevBuf<float> out;  // affine / softmax output [rows x pad4(dout)]
  // operand bounds of the two-plane GEMMs (Net::amax): per row / per column of the weights, the input activation, the gradient
  struct Bounds { DevBuf<float> rows, cols; } bw, bx, bd;
  // Dropout options of BiLstm(Parallel) in model-file token order (bilstm-layer.h:331-373): ForwardDropoutFactor,
  // ForwardTimeStepDropout, ForwardSequenceDropout, RecurrentTimeStepDropout, RecurrentSequenceDropout, RNNDrop,
  // NoMemLossDropout, RecurrentDropoutFactor, TwiddleForward (booleans stored as 0 / 1)
  float drop[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  bool has_dropout() const { return drop[0] > 0.f || drop[5] != 0.f || drop[6] != 0.f; }
  DevBuf<float> fmask;  // forward-dropout mask [T*S x ndir*H] of the current minibatch
  DevBuf<float> rmask;  // recurrent-dropout mask [(T+2)*S x ndir*H], indexed like C
  DevBuf<float> Yd;     // layer output after forward dropout [T*S x ndir*H]
  // what the last Propagate applied (Backpropagate must use the same, :888-889)
  bool cur_fwd_drop = false;
  int cur_drop_mode = 0;   // 0 none, 1 no-memory-loss, 2 RNNDrop
  bool cur_twiddle_coin = false;
  // one-shot injected masks (tests pin the kernels against the oracle with IDENTICAL masks): host copies until Propagate
  std::vector<float> inj_fmask, inj_rmask;
  int inj_rmask_rows = 0, inj_coin = -1;
  // the activation the next layer (and this layer's consumers) read
  const float* output(int S) const { return cur_fwd_drop ? Yd.p : Y.p + (size_t)S * ndir * H; }
  bool is_lstm() const { return kind == EESEN_LAYER_LSTM_PARALLEL || kind == EESEN_LAYER_BILSTM_PARALLEL; }
  bool nonparallel = false;  // read from a <BiLstm> / <Lstm> marker (Net::Write keeps the layer's own marker, layer.cc:37-46)
  bool is_activation() const { return kind == EESEN_LAYER_SIGMOID || kind == EESEN_LAYER_TANH; }
  bool trainable() const { return is_lstm() || kind == EESEN_LAYER_AFFINE; }
  long file_params() const;
  const char* marker() const;  // Layer::TypeToMarker (layer.cc:37-46, 68-79): the token the model file carries for this layer
};

class PhaseTimer {
 public:
  void enable(bool on) { on_ = on; }
  bool enabled() const { return on_; }
  // accumulate: spans pile up over several steps and are summed (and cleared) by one collect() -- no host
  // synchronisation per step is needed to time a multi-step region
  void set_accumulate(bool a) { accumulate_ = a; used_ = 0; }
  void reset() { if (!accumulate_) used_ = 0; }
  int begin(hipStream_t st, int phase);  // returns a span index (-1 when disabled)
  void end(hipStream_t st, int idx);
  void collect(float* out, int nphase);  // seconds per phase; synchronises on the recorded events
  int spans(int* phases, float* secs, int cap);  // every recorded span in record order (phase, seconds); does not clear
 private:
  struct Span { DevEvent a{true}, b{true}; int phase = 0; };
  std::vector<Span> spans_;
  size_t used_ = 0;
  bool on_ = false, accumulate_ = false;
};

// The phase times of one entry point of a loss object, in the two modes of eesen_ctc_set_profiling / eesen_ce_set_profiling.  The
// last call's (the default): one event per phase boundary, adjacent phases share one.  Accumulating (mode 2): a begin / end pair per
// phase, summed over the calls since the last read and cleared by it -- no synchronisation per call.
class PhaseClock {
 public:
  static constexpr int kMaxPhases = 3;
  void set_mode(bool accumulate) { spans_.enable(accumulate); spans_.set_accumulate(accumulate); }
  void mark(hipStream_t st, int phase);  // `phase` starts here (0 first, then in order); the one before it ends
  void stop(hipStream_t st);             // the last phase ends
  void read(float* out, int nphase);     // seconds per phase; waits for the recorded events
 private:
  DevEvent ev_[kMaxPhases + 1] = {DevEvent(true), DevEvent(true), DevEvent(true), DevEvent(true)};
  PhaseTimer spans_;
  int phase_ = 0, span_ = -1;
};

struct Comm;  // comm.cpp: RCCL communicator (one rank per GPU)
void comm_check_alive(const Comm* c);  // throws EESEN_ERR_COMM once the communicator's watchdog has aborted it (null: no-op)
constexpr size_t kLiveWords = 4;       // floats behind the gradient buffer: [0] = the data-parallel liveness word (comm.cpp)
// registers per SIMD lane one RCCL all-reduce workgroup needs to become resident on a CU: ncclDevKernel_Generic_{1,2,4} are 512-thread
// workgroups (two waves per SIMD) of 248-256 registers per lane -- at 256 threads per block one wave per SIMD: 256
// (profiles/r05_rccl_kernel_descriptors.md, read from librccl's gfx950 code object)
constexpr int kRcclVgprsPerSimdLane = 256;

// The hook of a loss object (Ctc, CeLoss) onto the error word of the Net whose outputs it evaluates (eesen_ctc_set_guard /
// eesen_ce_set_guard).  The word's value travels back with every minibatch's results; a minibatch computed while it was set (a
// timed-out persistent forward pass: garbage activations) is DROPPED from the statistics instead of being folded into them.
// Whichever of the two objects dies first undoes the hook.
struct StatGuard {
  const unsigned* word = nullptr;
  struct Net* net = nullptr;   // whose error word `word` points at
  long dropped = 0;
  hipStream_t st = nullptr;    // the loss object's stream: ~Net drains it before the word is freed
  StatGuard() = default;
  StatGuard(const StatGuard&) = delete;
  StatGuard& operator=(const StatGuard&) = delete;
  ~StatGuard() { unhook(); }
  void hook(struct Net* n, int device, hipStream_t stream, const char* entry_point);   // n == nullptr: only unhooks
  void unhook();
  void note_dropped(const char* what);   // counts, and warns at the first and every hundredth
  // A result's way back: `bytes` at `dev` into `pin` in stream order, a zero word behind them and -- hooked, and unless the caller
  // opts out -- the guard word's value of that moment copied over it.  Returns the host block; pin.wait() before it is read.
  void* read_back(PinBuf& pin, const void* dev, size_t bytes, hipStream_t stream, bool guarded = true);
  // Was the word raised behind the `bytes` of a block read_back returned?  Then they were computed from a timed-out forward pass:
  // NaN / -1 for the caller and nothing for the statistics, never garbage with status OK.
  static bool raised(const void* host, size_t bytes);
};

struct Net {
  int device = 0;
  hipStream_t st = nullptr;   // the caller's (NULL: the device's default stream); not owned
  std::vector<Layer> layers;
  bool finalized = false;
  size_t P = 0;  // floats in the flat buffers (with alignment padding)
  DevBuf<float> params, corr, fresh;
  float lr = 0.f, mmt = 0.f;
  // UpdateRule (trainable-layer.h:38) + NetTrainOptions::adagrad_epsilon / rmsprop_rho (train-opts.h:33-42)
  int rule = 0;  // 0 SGD, 1 Adagrad, 2 RMSProp
  float ada_eps = 1e-6f, rms_rho = 0.9f, rms_one_minus_rho = 0.1f;
  DevBuf<float> accu;         // squared-gradient accumulators, parameter layout; allocated on first use / Read
  bool accu_init = false;
  void init_accu();
  void set_accu(const float* host, long n);
  // current minibatch
  std::vector<int> lens;
  DevBuf<int> lens_d;
  int T = 0, S = 0, rows = 0;
  bool propagated = false;
  DevBuf<float> input;  // [rows x pad4(din0)]
  PinBuf in_stage[2];   // pinned staging of HOST inputs
  unsigned in_stage_idx = 0;
  const float* out_ptr = nullptr;
  int out_cols = 0, out_ld = 0;
  DevBuf<float> out_f;   // the net's output in the FILE's columns when the last layer is an LSTM layer padded to a multiple of 4 cells (forward_pass)
  // backward scratch
  DevBuf<float> DGb[2], DCF, dA, dB, ws, ws2;
  DevBuf<float> bwd_px;       // partial-sum exchange space of the K-split backward kernel (wide layers)
  DevBuf<float> bwd_dgh, bwd_ex;   // ... of its fp16-plane form: the gate gradients as planes, the inverse powers (LstmLayerDev::DGH / EX)
  DevStream st2;              // side stream: weight-gradient GEMMs under the next layer's recurrence
  DevEvent ev_rec, ev_grad[2];
  bool overlap = true;
  DevEvent ev_gate_reset, ev_gate_done;  // gated / early input GEMM of the next layer (forward)
  DevBuf<unsigned> mile;      // progress milestone of the running forward recurrence (LstmLayerDev::milestone) and the row guards of the next
                              // one (LstmLayerDev::guard): two regions of kMileRegion words, taken in turn by the layers (forward_pass)
  static constexpr int kMileRegion = 64, kGuardWord = 32;
  DevEvent ev_quad_go, ev_quad_done;   // "only the needed quadrants first": the recurrence below is through (main -> side); the deferred quadrants are in (side -> main)
  // The early forms of the NEXT layer's input GEMM that may run beside / behind LSTM layer li's forward recurrence (plan `fp`, T frames),
  // and which rows the early middle covers; and whether layer li, whose input GEMM's middle rows [r0, r1) are on the side stream, starts
  // its own recurrence (plan `fp`) behind two quadrants only.  ONE rule each for forward_pass and plan_string.
  struct FwdEarly { bool gate = false, mid = false; int mile_step = 0, r0 = 0, r1 = 0; };
  FwdEarly fwd_early(int li, const RecPlan& fp, int T) const;
  bool fwd_quad_rule(int li, const RecPlan& fp, int T, int r0, int r1, int steps[2]) const;
  bool gate_fwd = true;
  bool fwd_bf16 = false;      // eesen_net_set_forward_precision(1 | 2): forward GEMMs on bf16-rounded operands (BASELINE config 4)
  bool fwd_bf16_rec = false;  // ... (1 only): and the forward time recurrence on one bf16 plane of W_m / a bf16 exchange of m_t (lstm_fwd_persistent_bf16_kernel)
  int info_fwd_bf16 = 0;      // layers of the last Propagate whose recurrence ran on that kernel
  DevBuf<unsigned> ctl;       // arrival counters of the persistent recurrence kernels + [last] error word
  Tuning tn;                  // every run-time switch, read from the environment when the Net is created (tuning.h)
  int persistent = 1;         // EESEN_PERSISTENT=0 forces the one-launch-per-step kernels; also cleared by a recovery
  int info_fwd_persistent = 0, info_bwd_persistent = 0, info_lstm_layers = 0;   // of the last Propagate / Backpropagate (tests)
  int spin_limit = 400000;
  float flight_ns = 0.f;      // measured increment flight between two CUs of this device
  int delay_fwd = 61, delay_bwd = 43, delay_bwd_side = 64, poll_raw = 0;   // first-poll delays derived from it, wall-clock ticks of 10 ns
  int recoveries = 0;         // times a timed-out persistent kernel made the net fall back to the per-step kernels
  DevBuf<unsigned long long> trace;  // EESEN_TRACE=1 debug timeline
  void check_device_error(bool consumer);
  int steps_since_clean = 0;  // Propagates enqueued since the error word was last seen clear
  // set_seq_lengths does not drain the stream: the lengths go through a PinBuf (the previous copy has long completed; waiting
  // for it bounds the host's run-ahead to one step), and the persistent kernels' error word is polled through an asynchronous
  // copy into another, enqueued behind every Propagate / Update (full check in sync()).
  PinBuf lens_pin, err_pin;
  bool err_armed = false;
  void poll_device_error();      // non-blocking
  void arm_device_error_poll();  // enqueue the copy of the error word
  // dropout
  bool in_train = true;                       // BiLstm::in_train (bilstm-layer.h:38), Net::SetTrainMode / SetTestMode
  unsigned long long drop_seed = 777, drop_counter = 0;   // masks are a pure function of (seed, draw counter, element)
  void set_train_mode(bool train) { in_train = train; }
  // eesen_net_debug_layer_buffer (test hook): which LSTM layer's gate gradients each of the two DGb slots holds since the last
  // Backpropagate (-1: none; cleared by Propagate), and the read-out itself
  int dg_owner[2] = {-1, -1};
  void debug_layer_buffer(int layer, int which, float* host, long cap_floats, int* rows_out, int* cols_out);
  void set_layer_dropout(int layer, const float* nine);
  void get_layer_dropout(int layer, float* nine) const;
  void set_dropout_masks(int layer, const float* fwd, long fwd_n, const float* rec, int rec_rows, long rec_n, int coin);
  void get_dropout_masks(int layer, float* fwd_host, float* rec_host, int* info4);
  size_t ws_floats = 0;
  // Operand bounds of the two-plane fp16 GEMMs (gemm.hip, mode 2; kernels.h: GemmBound).  Every GEMM operand is scaled per row of
  // op(A) / column of op(B) by the power of two that its own bound asks for, so a dot product's precision does not depend on what
  // the rest of the tensor holds.  Per layer (Layer::bw / bx / bd): the bounds of the rows AND of the columns of [W] the weight matrix
  // its GEMMs multiply with (W_x / W; measured after every parameter change), [X] its input activation (measured in Propagate where the
  // structure gives no bound, reused by Backpropagate), [D] the gradient it multiplies in Backpropagate (DG of an LSTM layer, out_diff
  // of an affine one) -- one pass per tensor (amax_rows_cols).  What the structure bounds takes one word: `amax[0]` = 1.0 for LSTM
  // outputs (|m| = |o tanh c| < 1) and sigmoid / tanh / softmax outputs.  amax[1 + li]: max |W_m| of LSTM layer li (the fp16-plane
  // forward recurrence, lstm_persistent.hip).  The GEMM of a PART of a tensor takes the same words, so results do not depend on how a
  // GEMM is cut.
  DevBuf<float> amax, amax_ws;
  bool wamax_valid = false, wm_valid = false;
  bool amx_valid = false;     // the [X] bounds are those of the last Propagate
  float* am_wm(int li) { return amax.p + 1 + li; }
  GemmBound bound_one() const { return GemmBound{amax.p, 0}; }
  bool x_is_bounded(int li) const;                    // layer li's input needs no measurement (bounded by 1)
  void measure(const float* P, long rows, int cols, int ld, DevBuf<float>& out_rows, DevBuf<float>& out_cols);
  void ensure_weight_amax();
  PhaseTimer timer;
  // data-parallel exchange (comm.cpp): with a communicator attached, Backpropagate sums every layer's fresh gradients
  // over the ranks on the communicator's stream as soon as that layer's weight-gradient kernels are enqueued (the point
  // of the reference's per-layer Update, net.cc:98-104), and Update waits bucket by bucket
  Comm* comm = nullptr;                       // not owned
  std::vector<DevEvent> ev_ready, ev_bucket;
  std::vector<char> bucket_pending;
  // EESEN_COMM_DEFER=1 (tuning.h): the buckets of a backward pass are issued when its last recurrence has run instead of as each
  // layer's gradients are enqueued -- no all-reduce kernel then competes with a persistent grid for CUs (comm.cpp)
  std::vector<int> deferred_buckets;
  bool exchange_deferred = false;             // this backward pass's schedule (decided per minibatch: exchange_deferred_for_minibatch)
  std::vector<RecPlan> bwd_plans(int T) const;   // per layer: the backward recurrence plan at the current shape and T frames (net.cpp)
  bool overlap_for_minibatch(const std::vector<RecPlan>& bwd) const;   // weight-gradient GEMMs on the side stream for the current shape
  bool exchange_deferred_for_minibatch(const std::vector<RecPlan>& bwd) const;
  std::string plan_string() const;            // eesen_net_plan_string
  DevEvent ev_bwd_done;
  void issue_bucket(int li);
  void fail_step_buckets() noexcept;          // Backpropagate threw with peers waiting: complete the step's collective sequence (comm.cpp)
  void flush_deferred_buckets();
  std::vector<StatGuard*> guards;   // the loss objects guarding on this Net's error word (eesen_ctc_set_guard / eesen_ce_set_guard): unhooked in ~Net
  bool grads_sanitized = false;   // this step's gradients went through an all-reduce that zeroed them on a raised error word: update() must apply
  bool live_valid = false;        // the liveness word behind the gradient buffer was written for THIS step (backpropagate / backpropagate_zero)
  std::vector<int> bucket_log;                // layer order of the last Backpropagate's buckets (tests)
  PinBuf live_pin;                            // landing slot of the liveness word
  void set_comm(Comm* c);
  int top_trainable() const;
  int live_ranks();
  void bucket_allreduce(int li, hipStream_t producer);   // (deferred with EESEN_COMM_DEFER=1: see flush_deferred_buckets)
  void wait_buckets_host();
  void backpropagate_zero();
  void allreduce_grads(Comm* c);

  Net(int device, void* stream);
  ~Net();
  void add_layer(int kind, int din, int dout, float coef, float max_grad);
  void finalize();
  long num_params() const;
  void set_params(const float* host, long n);
  void get_flat(const DevBuf<float>& buf, float* host, long n);  // params or fresh grads in Net::GetParams order
  void set_seq_lengths(const int* lens, int S);
  void propagate(const float* in, int rows, int ld, bool is_device);
  void forward_pass();
  void backpropagate(const float* out_diff, int ldd, float* in_diff, int ldi);
  void backpropagate_impl(const float* out_diff, int ldd, float* in_diff, int ldi);
  void update();
  void refresh_derived();  // W_m^T copies
  // MomentStatistics (utils-functions.h:50-82) of the tensors of one layer in the reference's Info() / InfoGradient() order
  // (bilstm-layer.h:496-560, lstm-layer.h:175-196, affine-trans-layer.h:145-159).  which: 0 parameters, 1 the momentum
  // buffers (*_corr_), 2 the adaptive accumulators (*_corr_accu; zeros until an adaptive rule ran).  Returns the tensor count.
  int tensor_moments(int which, int layer, double* out6_host, int cap_tensors);
  void read(const std::string& path);
  void write(const std::string& path, bool binary);
  void sync();
};

// a staging / result slot of the loss objects: twice what is asked for when it has to grow, at least a page
inline void* loss_slot(PinBuf& pin, size_t bytes) { return pin.reserve(bytes, std::max<size_t>(bytes * 2, 4096)); }

// Staging of the loss objects' small inputs (labels, lengths, targets): n ints, written by fill(pinned), to `dst` on the device through
// two alternating pinned slots.  The upload is stream-ordered: kernels of the previous call that still read `dst` are ahead of this
// copy on the stream, and the slot written here was last read by the copy of two calls ago -- nothing drains the stream.
struct StageSlots {
  PinBuf slot[2];
  unsigned idx = 0;
  template <class Fill> void upload(hipStream_t st, int* dst, size_t n, Fill&& fill) {
    PinBuf& sp = slot[idx++ & 1];
    int* pinned = static_cast<int*>(loss_slot(sp, n * sizeof(int)));
    fill(pinned);
    EESEN_HIP_CHECK(hipMemcpyAsync(dst, pinned, n * sizeof(int), hipMemcpyHostToDevice, st));
    sp.used(st);
  }
};

// The shape every entry point of the loss objects takes: rows = T * S, ld >= K, 0 <= frame_num_utt[s] <= T.  min_K: 2 the decoder, 1 the
// losses and the alignment, 0 the callers that refuse K <= 0 as a short leading dimension.
void check_shape(const int* frame_num_utt, int S, int rows, int K, int ld, int min_K);

struct Ctc {
  int device = 0;
  hipStream_t st = nullptr;
  DevBuf<float> logp, alpha, beta, pzx_d;
  DevBuf<int> labx, ids_d, ali_d;   // ali_d: class ids [rows], lattice positions [rows], then the scores [S] of align_parallel
  std::vector<int> last_lens;
  int last_T = 0, last_S = 0, last_Lpad = 0, last_Lprime = 0;
  int sweep_waves = 0;   // EESEN_CTC_WAVES when this object was created (tuning.h): 0 = the default number of waves per lattice
  double obj_sum = 0;
  long sequences = 0, frames = 0, err_tokens = 0, ref_tokens = 0;
  PhaseClock clock;            // eval_parallel (phases: log, alpha / beta, error signal)
  PhaseClock align_clock;      // align_parallel (phases: log, sweep, traceback)
  PinBuf align_pin;            // results of align_parallel (D2H)
  // decode_parallel (ctc_decode.hip): candidates of every frame and the final beam (floats, ints), the trie, the hypotheses
  DevBuf<float> dec_f;
  DevBuf<int> dec_i, dec_trie, dec_out;
  PhaseClock decode_clock;     // phases: top-C (with the logarithm), beam, hypotheses
  PinBuf decode_pin;           // results of decode_parallel (D2H): dec_out as it is, then the guard word
  // What the last decode call left for get_decode_candidates, decode_stamps, decode_rescore and decode_mbr: where everything is (dec),
  // the candidates in dec_f / dec_i, the hypotheses in dec_out (device) and in decode_pin (host), until the next decode call.
  DecodeLayout dec;
  std::vector<int> dec_lens;
  int dec_space = -1;          // the space class of a spaced lexicon, -1 in every other mode
  // whose ids the LM tokens of an entry are: 0 its labels (plain, token LM), 1 a spaced lexicon's words (in dec_word / dec_word_len:
  // the lexicon may be gone by then), 2 an unspaced lexicon's (words and word ends in dec_out)
  int dec_tokens() const { return dec.mode == kDecodeWords ? 2 : dec_space >= 0 ? 1 : 0; }
  std::vector<int> dec_word, dec_word_len;   // [S * N * T], [S * N]
  DevBuf<int> stamp_i;         // decode_stamps: lattices, per-lattice lengths, positions, then the results (label starts, ends, path scores)
  PhaseClock stamp_clock;      // phases: lattice build (with the logarithm), sweep + traceback, stamps
  PinBuf stamp_pin;            // results of decode_stamps (D2H)
  int stamp_group = 0;         // eesen_ctc_set_stamp_group: lattices per sweep launch, 0 = as many as kStampDeltaBytes holds (tuning.h)
  // score_parallel / decode_rescore (INTEGRATION.md "Rescoring"): lattices, expanded-label lengths, frame counts and utterance of
  // every lattice, then the scores.  Nothing else: the scoring sweep keeps no row
  DevBuf<int> score_i;
  PhaseClock rescore_clock;    // rescore_times: lattice build (+ log), sweep; always the last call's
  double rescore_host_s = 0;   // ... and the host's LM scoring and ranking of the last decode_rescore
  PinBuf score_pin;            // results of the scoring sweep (D2H)
  int dec_V = 0;               // the lexicon's word count of the last decode call (0: none): what a second word LM must fit
  // edit_distance_parallel / decode_mbr (INTEGRATION.md "Minimum Bayes risk"): uploaded tokens, jobs, then the distances
  DevBuf<int> ed_i;
  PinBuf ed_pin;               // the distances and the guard word (D2H)
  DevEvent mev[2] = {DevEvent(true), DevEvent(true)};   // around the distance kernel
  double mbr_t[3] = {0, 0, 0}; // mbr_times: job build + uploads, the kernel, the host's posterior / risk / ranking
  bool mbr_accumulate = false; // eesen_ctc_set_profiling(2): the three are summed over the calls until they are read
  // the tables of the token LM the last decode_parallel_lm used (lm.h), keyed by the model's serial
  DevBuf<int> lm_i;
  DevBuf<float> lm_f;
  LmTables lm_tab{};
  unsigned long long lm_serial = 0;
  // the tables of the lexicon the last decode_parallel_lex used (lex.h), keyed in the same way
  DevBuf<int> lex_i;
  LexTables lex_tab{};
  WordLexTables word_tab{};    // ... of an unspaced lexicon (decode_parallel_words): the same buffer and serial
  unsigned long long lex_serial = 0;
  // the unigram look-ahead (eesen_ctc_set_lm_lookahead; INTEGRATION.md "LM look-ahead"): 0 off, 1 unigram.  The table of the
  // (lexicon, word LM) pair the last look-ahead decode used, keyed by the two serials
  int lm_lookahead = 0;
  DevBuf<float> la_f;          // [nodes], then [edges]: la of every edge's target
  unsigned long long la_lex_serial = 0, la_lm_serial = 0;
  // Nothing in a training step has to stall the host: label staging goes through two alternating PinBufs, and the
  // per-sequence ln p / the greedy-decode ids of a call whose caller did not ask for them (NULL result pointers) come
  // back through PinBufs that are folded into the statistics at the next call that needs them ("deferred").
  StageSlots stage;            // label expansion, lengths, tokens and jobs (H2D)
  struct PendingPzx { PinBuf pin; int S = 0; long nframes = 0; bool active = false; } ppzx[2];
  struct PendingErr { PinBuf pin, probs; int S = 0, K = 0, rows = 0; bool active = false, with_probs = false; std::vector<int> frames, ids, off; } perr[2];
  StatGuard guard;             // eesen_ctc_set_guard
  std::string seq_out;         // --sequence-out-file of the trainer (ctc-loss.cc:247-250,282-291): decoded sequences are appended here
  unsigned ppzx_idx = 0, perr_idx = 0;
  void flush_pzx(PendingPzx& q);
  void flush_err(PendingErr& q, int* num_err, int* num_ref);
  void flush();                // fold every deferred result into the statistics (blocks until they have arrived)

  Ctc(int device, void* stream);
  ~Ctc();
  void eval_parallel(const int* frame_num_utt, int S, const float* net_out, int rows, int K, int ld, const int* label_ids,
                     const int* label_off, float* diff, int ldd, float* pzx_host);
  void error_rate_mseq(const int* frame_num_utt, int S, const float* net_out, int rows, int K, int ld,
                       const int* label_ids, const int* label_off, int* num_err, int* num_ref);
  void get_alpha_beta(float* alpha_host, float* beta_host, int* Lprime);
  void set_profiling(int mode);   // eesen_ctc_set_profiling: 2 = the phase clocks and the MBR times accumulate until they are read
  void phase_times(float* out3) { clock.read(out3, 3); }
  // Best-path alignment (ctc_best_path + ctc_traceback in ctc.hip); touches neither the objective nor the error statistics.
  void align_parallel(const int* frame_num_utt, int S, const float* scores, int rows, int K, int ld, bool is_log, const int* label_ids,
                      const int* label_off, int* ali_host, int* pos_host, float* score_host);
  void align_times(float* out3) { align_clock.read(out3, 3); }
  // Prefix beam search over the posteriors (ctc_row_topc + ctc_prefix_beam + ctc_hyp in ctc_decode.hip); touches neither the
  // objective nor the error statistics, and none of the buffers of eval_parallel / align_parallel but `logp`.
  void decode_parallel(const int* frame_num_utt, int S, const float* scores, int rows, int K, int ld, bool is_log, int beam, int max_classes,
                       int nbest, int* hyp_host, int* hyp_len_host, float* score_host);
  // the same with a token n-gram LM fused into the beam (ctc_prefix_beam with its tables); lm_score_host [S][nbest] may be null
  void decode_parallel_lm(const int* frame_num_utt, int S, const float* scores, int rows, int K, int ld, bool is_log, int beam, int max_classes,
                          int nbest, const TokenLm* lm, float lm_weight, float insertion_bonus, bool use_eos, int* hyp_host, int* hyp_len_host,
                          float* score_host, float* lm_score_host);
  // the search along a lexicon trie, with or without (lm == null) an LM over its word ids; word_host [S][nbest][T] / word_len_host
  // [S][nbest]: the segmentation of every returned labelling (Lexicon::words on the host), -1 beyond; either may be null
  void decode_parallel_lex(const int* frame_num_utt, int S, const float* scores, int rows, int K, int ld, bool is_log, int beam, int max_classes,
                           int nbest, const Lexicon* lex, const TokenLm* lm, float lm_weight, float word_bonus, bool use_eos, int* hyp_host,
                           int* hyp_len_host, float* score_host, float* lm_score_host, int* word_host, int* word_len_host);
  // the word beam search along an unspaced lexicon (ctc_word_beam + ctc_word_hyp in ctc_decode.hip): hypotheses are labels and
  // the words closed between them; words, word counts and word ends (word_end_host [S][nbest][T]: labels up to and including word
  // j's last) come from the device; the three may be null
  void decode_parallel_words(const int* frame_num_utt, int S, const float* scores, int rows, int K, int ld, bool is_log, int beam, int max_classes,
                             int nbest, const Lexicon* lex, const TokenLm* lm, float lm_weight, float word_bonus, bool use_eos, int* hyp_host,
                             int* hyp_len_host, float* score_host, float* lm_score_host, int* word_host, int* word_len_host, int* word_end_host);
  void decode_times(float* out3) { decode_clock.read(out3, 3); }
  // Time stamps and confidences of the last decode call's entries (INTEGRATION.md "Time stamps and CTM"): ctc_hyp_lattices, then
  // ctc_best_path + ctc_traceback over all S * nbest lattices in groups, then ctc_stamp; words and confidences on the host.
  // lstart / lend / wstart / wend (int) and wconf (float) [S][nbest][T], path_score [S][nbest]; any may be null.
  void decode_stamps(const int* frame_num_utt, int S, const float* scores, int rows, int K, int ld, bool is_log, double conf_scale,
                     int* lstart_host, int* lend_host, int* wstart_host, int* wend_host, float* wconf_host, float* path_score_host);
  void stamp_times(float* out3) { stamp_clock.read(out3, 3); }
  // Exact log-scores ln p(labels | x) (INTEGRATION.md "Rescoring"; ctc_score in ctc.hip): utterance s has the labellings
  // hyp_off[s] .. hyp_off[s + 1], labelling h the labels label_ids[label_off[h] .. label_off[h + 1]) (none: the empty labelling).
  // Touches neither the statistics nor the lattices of the last eval_parallel; the logarithms borrow `logp`.
  void score_parallel(const int* frame_num_utt, int S, const float* scores, int rows, int K, int ld, bool is_log, const int* hyp_off,
                      const int* label_off, const int* label_ids, float* score_host);
  // The last decode call's entries scored exactly and ranked again: total = am + lm_weight * g + bonus * n with g the second LM's
  // fp64 score of the entry's LM tokens (lm == null: the first pass's LM sum).  am / lm / total (float) and order (int) [S][nbest];
  // any may be null.  Leaves what the decode call left untouched.
  void decode_rescore(const int* frame_num_utt, int S, const float* scores, int rows, int K, int ld, bool is_log, const TokenLm* lm,
                      float lm_weight, float bonus, bool use_eos, float* am_host, float* lm_host, float* total_host, int* order_host);
  void rescore_times(float* out3) { rescore_clock.read(out3, 2); out3[2] = (float)rescore_host_s; }
  // Levenshtein distances on the device (edit_distance_jobs in edit_distance.hip), every integer equal to edit_distance() below.
  // Group g owns the sequences seq_off[g] .. seq_off[g + 1], sequence q the tokens tok_ids[tok_off[q] .. tok_off[q + 1]); pair_host:
  // n_g x n_g distances per group, packed; ref_dist_host [NQ]: every sequence against its group's reference.  No statistic touched.
  void edit_distance_parallel(int G, const int* seq_off, const int* tok_off, const int* tok_ids, const int* ref_off, const int* ref_ids,
                              int* pair_host, int* ref_dist_host);
  // Minimum Bayes risk over the last decode call's entries: pairwise distances [S][nbest][nbest], distances to the references
  // [S][nbest], posteriors and expected errors (double) [S][nbest], and the ranks by expected errors [S][nbest]; any may be null.
  // level 0: the mode's LM tokens, 1: labels.  z: total_host if given, else the decode call's scores.  Leaves what that call left.
  void decode_mbr(int S, int level, double scale, const float* total_host, const int* ref_off, const int* ref_ids, int* dist_host,
                  int* ref_dist_host, double* post_host, double* risk_host, int* order_host);
  void mbr_times(float* out3);
  // the candidate classes the last decode_parallel selected: ids / scores [rows][C'], blank [rows]; rows beyond an utterance: -1 / -1e30
  void get_decode_candidates(int* ids_host, float* scores_host, float* blank_host, int* Cc);
 private:
  struct Lattices { const int *labx, *lens, *lablens; int Lpad, Lprime; };
  Lattices upload_lattices(const int* frame_num_utt, int S, const int* label_ids, const int* label_off);
  void decode_batch(const int* frame_num_utt, int S, const float* scores, int rows, int K, int ld, bool is_log, int beam, int max_classes,
                    int nbest, const Lexicon* lex, const TokenLm* lm, float lm_weight, float bonus, bool use_eos, int* hyp_host, int* hyp_len_host,
                    float* score_host, float* lm_score_host, int* word_host, int* word_len_host, int* word_end_host);
  void upload_lm(const TokenLm& lm);
  void upload_lex(const Lexicon& lex);
  const float* upload_lookahead(const Lexicon* lex, const TokenLm* lm);   // null with the mode off; refuses a missing word LM
  // The distances of `jobs` ([n][4], kernels.h) through ed_i and ed_pin.  tok_h [n_tok] is uploaded.  Jobs [0, n_same) take both spans
  // from dev_tok (null: the uploaded array), the others their first span from there and their second from the uploaded array.
  // Returns the pinned results, *bad = the guard word's value behind them (bad == null: not read); adds its times to mbr_t[0] and [1].
  const int* ed_run(const int* tok_h, size_t n_tok, const int* dev_tok, const std::vector<int>& jobs, size_t n_same, int max_len, bool* bad);
};

// N-best posterior word confidences (eesen_word_confidence; INTEGRATION.md "Time stamps and CTM"), fp64, no device work.  Entry i of
// n has total scores[i] and word_len[i] words (< 0: not an entry) with ids / intervals [wstart, wend) in rows of `stride`.
// conf_out [n][stride]: sum over the entries k that hold a word of the same id whose interval intersects, of P_k = softmax(c * scores)_k;
// -1e30 beyond an entry's words.
void word_confidence(int n, const double* scores, const int* word_len, const int* word_ids, const int* wstart, const int* wend, int stride,
                     double conf_scale, double* conf_out);

// LevenshteinEditDistance (src/util/edit-distance-inl.h), total errors only: what Ctc::error_rate_mseq counts with (ctc_host.cpp)
int edit_distance(const int* ref, int nr, const int* hyp, int nh);

// eesen::CE (src/net/ce-loss.h:32-77): frame-level cross-entropy (ce_host.cpp, ce.hip).  As with the Ctc nothing in a training
// step stalls the host: targets travel through two alternating PinBufs, and each call's sums come back through a PinBuf
// that is folded into the running totals -- in call order -- when the next-but-one call needs the slot or the totals are read.
struct CeLoss {
  int device = 0;
  hipStream_t st = nullptr;
  DevBuf<int> tg;              // lens[S] then targets[rows] of the current call
  DevBuf<CeSums> part, res;    // workgroup partials, the call's sums
  StageSlots stage;
  struct Pending { PinBuf pin; int S = 0; long rows = 0; bool active = false; } pend[2];
  unsigned pend_idx = 0;
  // running totals and the *_progress_ counters of ce-loss.cc:144-167 (the reference's are int32; these are wide)
  double obj = 0, obj_progress = 0;
  long correct = 0, frames = 0, sequences = 0, correct_progress = 0, frames_progress = 0, sequences_progress = 0;
  int report_step = 100;       // the trainer's default (train-ce-parallel.cc:52); the reference's CE leaves it uninitialised
  std::vector<std::string> progress;   // progress lines not yet handed out (eesen_ce_progress), oldest first
  StatGuard guard;             // eesen_ce_set_guard
  PhaseClock clock;            // one phase: ce_eval

  CeLoss(int device, void* stream);
  ~CeLoss();
  void fold(Pending& q, double* obj_out);
  void flush();                // fold every pending call into the totals (blocks until their sums have arrived)
  void eval_parallel(const int* frame_num_utt, int S, const float* net_out, int rows, int K, int ld, const int* targets,
                     float* diff, int ldd, double* obj_host);
  std::string report();
  void phase_times(float* out1) { clock.read(out1, 1); }
};

}  // namespace eesen
