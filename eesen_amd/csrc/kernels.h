// kernels.h -- host-side launchers of the gfx950 kernels (definitions in gemm.hip, lstm.hip, ctc.hip, optim.hip).
// All pointers are device pointers; every launcher enqueues on `st` and returns without synchronising.
#pragma once
#include "common.h"

namespace eesen {

// ---------------------------------------------------------------------------------------- gemm.hip
// C[M x N] = alpha * op(A) * op(B) + beta * C (+ bias[n]).  fp32 in, fp32 accumulate on
// v_mfma_f32_32x32x2_f32.  a_kc: A stored [M x K] (k contiguous) else [K x M]; b_kc: B stored [N x K]
// else [K x N].  All base pointers 16-byte aligned and all leading dimensions multiples of 4.
// `ws`/`ws_floats`: split-K workspace (may be null => no split).  Replaces the cublasSgemm behind
// CuMatrixBase::AddMatMat (/root/reference/src/gpucompute/cuda-matrix.cc:604-639).
// Mode 2 (two fp16 planes): a bound of an operand's magnitudes, in device words -- per_index = 1: one word per M index of op(A) /
// N index of op(B) (the bound of that row / column: the scale is then the dot product's own), 0: one word for the whole operand.
// p = null: measured by a pass over the operand before the launch.  Ignored by the other modes.
struct GemmBound {
  const float* p = nullptr;
  int per_index = 0;
};
void gemm_f32(hipStream_t st, bool a_kc, bool b_kc, int M, int N, int K, float alpha, const float* A, int lda,
              const float* B, int ldb, float beta, float* C, int ldc, const float* bias, float* ws,
              size_t ws_floats, int extra_lds_bytes = 0,   // extra_lds_bytes: unused dynamic LDS = occupancy cap per CU
              bool bf16_operands = false,                  // round both operands to bf16, one bf16 MFMA product, fp32 accumulate
              GemmBound bound_a = {}, GemmBound bound_b = {});

// Arithmetic of every gemm_f32 / gemm_f32_nt_gated call: 0 = f32-input MFMA, 1 = 3-way bf16 split (six products), 2 = two fp16
// planes (three products; gemm.hip); -1 = follow EESEN_GEMM_MODE.  Process-wide.
constexpr int kDefaultGemmMode = 2;
int gemm_mode();
void set_gemm_mode(int mode);
// *out = max |P[r][c]| over a [rows x cols] matrix with row stride ld (amax_abs zeroes the word first; _accumulate folds into it)
void amax_abs(hipStream_t st, const float* P, long rows, int cols, int ld, float* out);
void amax_abs_accumulate(hipStream_t st, const float* P, long rows, int cols, int ld, float* out);
// one pass: out_rows[r] = max_c |P[r][c]| and / or out_cols[c] = max_r |P[r][c]| (either may be null; out_cols needs a workspace
// `ws` of kAmaxBlocks * min(16384, pad4(cols)) floats)
constexpr int kAmaxBlocks = 512;
void amax_rows_cols(hipStream_t st, const float* P, long rows, int cols, int ld, float* out_rows, float* out_cols, float* ws);

// Arrival counters of the persistent recurrence kernels (lstm_persistent.hip): per (direction, sequence tile) group 8
// shards (shard = blockIdx.x & 7), one 128-byte line each; a shard counts workgroups-in-shard x completed steps.
#ifndef EESEN_SHARDS
#define EESEN_SHARDS 8
#endif
constexpr int kShards = EESEN_SHARDS, kShardStride = 32;  // words
constexpr int kCtlHalf = 2048 * kShards;                  // words of counters per pass (forward / backward): 64 groups

// "Gated" input->gates GEMM: C = A * B^T + bias where the rows of A are the time-major output [T*S x K] of an LSTM layer
// whose persistent forward kernel is STILL RUNNING on another stream.  A tile of rows waits until the arrival counters
// say that both directions have passed its frames (forward direction: steps >= t_hi + 1, backward: steps >= T - t_lo);
// tiles are visited middle-out in time, which is the order in which a bidirectional layer completes frames.
struct GemmGate {
  const unsigned* cnt;  // counters of the producing kernel
  unsigned* err;        // raised when the bounded spin gives up
  int ndir, nz, nblk;   // counter groups (ndir x nz) and workgroups per group
  int T, S;
  int spin_limit;
};
void gemm_f32_nt_gated(hipStream_t st, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C,
                       int ldc, const float* bias, const GemmGate& gate, GemmBound bound_a = {}, GemmBound bound_b = {});

// ---------------------------------------------------------------------------------------- lstm.hip
struct LstmLayerDev {
  // geometry
  int T, S, H, ndir;
  // activations of this layer (see DESIGN.md "data layout")
  float* G;         // [T*S x ndir*4H]   gate-interleaved (col = dir*4H + u*4 + q, q in g,i,f,o)
  float* C;         // [(T+2)*S x ndir*H] cell state, row (t+1)*S+s, boundary row-blocks zero
  float* Y;         // [(T+2)*S x ndir*H] cell output m, same indexing; rows S.. are the layer output
  // Exchange copy of m for the persistent forward kernel (optional, may be null): the SAME values in the order the consumers
  // fetch them -- per (t, dir, 16-sequence tile) a block [chunk of 32 units][k half][k quad][16 sequences][4 floats], so that
  // 16 adjacent lanes of an operand load read 256 contiguous bytes (whole 128-byte lines, each requested once) instead of 16
  // bytes out of 16 different rows of Y.  T * ndir * ceil(S/16) * ceil(H/32) * 512 floats.
  float* X = nullptr;
  // parameters (internal layout)
  const float* Wm;   // [ndir][4H x H]   rows gate-interleaved (u*4+q)
  const float* WmT;  // [ndir][H x 4H]   transpose of the above
  const float* peep; // [ndir][3][H]     p_i, p_f, p_o
  const int* lens;   // [S]
  // recurrent dropout (bilstm-parallel-layer.h:209-377): mask of 0 / 1/(1-p), [(T+2)*S x ndir*H], indexed like C;
  // drop_mode 0 none, 1 no-memory-loss (mask multiplies g*i), 2 RNNDrop (mask multiplies the whole new cell)
  const float* rmask = nullptr;
  int drop_mode = 0;
  // sequence window of one persistent launch: sequences [s_begin, s_begin + s_count) of the S interleaved ones.  Shapes whose
  // whole batch needs more workgroups than can be co-resident (S = 64 at H = 1024: BASELINE config 5) run as several
  // launches, one window each -- the sequences are independent chains.  s_count = 0 means all S.
  int s_begin = 0, s_count = 0;
  // partial-sum exchange space of the K-split backward kernel for wide layers (what the backward plan asks for: RecPlan::need_px)
  float* PX = nullptr;
  size_t px_floats = 0;
  // first-poll delay of the persistent kernels' hand-off waits in wall-clock ticks of 10 ns; set by the host from the measured
  // increment flight of the device (handoff_flight_ns)
  int poll_delay = 0;
  int poll_raw = 0;   // 1: poll_delay is an experimenter's value (EESEN_POLL_NS): the launchers apply no per-plan factor to it
  // progress milestone of the narrow forward persistent kernel (null: none; two words): when every workgroup of a (direction, sequence
  // tile) group has published step `milestone_step`, the group's first workgroup adds 1 to milestone[0], and the last group sets
  // milestone[1] -- the host starts the GEMM that consumes this pass's rows for the frames both directions have finished by then
  // while the recurrence is still running (net.cpp: "the middle first")
  unsigned* milestone = nullptr;
  int milestone_step = 0;
  // row guards of the narrow forward persistent kernel (lstm_fwd_persistent_bf_guard_kernel, RecPlan::fn_guard; null / -1: none): rows
  // of G that another stream is still computing when the kernel is launched.  Before any workgroup touches the gate rows of step
  // guard_step[i] (>= 2) it waits until *guard[i] != 0; the host sets the word behind the GEMM that writes those rows (net.cpp: "only the needed quadrants first")
  const unsigned* guard[2] = {nullptr, nullptr};
  int guard_step[2] = {-1, -1};
  // kernel selection switches (tuning.h; all 1 in production): XCD-aware role map, time-multiplexed forward kernel, 4 x 32 and
  // K-split backward tiles
  int xcd_map = 1, fwd_mux = 1, bwd_q4 = 1, bwd_ksplit = 1, bwd_mux = 1;
  int fwd_t16_small = 1; // batches of <= 16 sequences on narrow layers: the 16 x 8 tile (bf16-pipe kernel) instead of the 32 x 4 fp32 tile (tuning.h: EESEN_FWD_T16_SMALL)
  int fwd_narrow2 = 1;  // the narrow bf16-pipe forward tile as up to two workgroups per CU where a census has seen them resident (tuning.h: EESEN_FWD_NARROW2)
  int bwd_q4_st8 = 1;   // the 4 x 32 backward tile with TWO 4-sequence tiles per workgroup where one does not fit (tuning.h: EESEN_BWD_Q4_ST8)
  // eesen_net_set_forward_precision(1): the recurrent product m_{t-1} W_m^T of the persistent forward kernel on bf16 operands with
  // fp32 accumulation (lstm_fwd_persistent_bf_kernel<.., AP = 1, WP = 2>): m_t as ONE bf16 plane in the exchange buffer X, W_m as
  // hi + lo planes
  int fwd_bf16 = 0;
  // fp32-class forward recurrence on the bf16 matrix pipe (3-way split of both operands, six products; tuning.h: EESEN_FWD_SPLIT)
  int fwd_split = 0;
  // fp32-class forward recurrence on TWO fp16 planes per operand, three products (round 6; tuning.h: EESEN_FWD_F16): taken where
  // the 3-way split would be, and on the wide 16 x 16 tile.  wm_amax: device word holding max |W_m| of this layer (both directions).
  int fwd_f16 = 0;
  const float* wm_amax = nullptr;
  // the K-split backward tile of wide layers on two fp16 planes per operand (round 6; tuning.h: EESEN_BWD_F16): DGH = the gate gradients a
  // second time, as planes with a per-(producer, sequence) power of two ([T*S x ndir*4H] words of 4 bytes: the fp32 rows' bytes), EX = the
  // inverse powers ([T][ndir][ceil(S/16)][H/16][4 groups of 4 sequences] words of 16 bytes); handed over when the backward plan asks (RecPlan::need_dgh, need_ex)
  int bwd_f16 = 0;
  unsigned char* DGH = nullptr;
  float* EX = nullptr;
};
float handoff_flight_ns();
// The share of the device's CUs this PROCESS sizes its persistent grids against: 1/n (EESEN_GPU_SHARE, or set by a communicator
// that found n of its ranks on this device: comm.cpp).  Process-wide.
void set_gpu_share(int n);
int gpu_share_value();
// one wave that returns once *word >= target (or when the recurrence kernels' error word is raised; it raises that word itself
// if it ever gives up): puts a stream behind a milestone of a kernel that is still running on another stream
void wait_for_word(hipStream_t st, const unsigned* word, unsigned target, unsigned* err, double limit_s = 2.0);   // gives up after limit_s seconds of wall clock
// One recurrence step of every direction: fw direction handles t = step, bw direction t = T-1-step.
void lstm_fwd_step(hipStream_t st, const LstmLayerDev& L, int step);
// One step of the backward recurrence: fw direction handles t = T-1-step, bw direction t = step.
// dY: [T*S x ndir*H] gradient w.r.t. the layer output, DG: [T*S x ndir*4H] (out), DCF: [S x ndir*H] carry.
void lstm_bwd_step(hipStream_t st, const LstmLayerDev& L, int step, const float* dY, int lddy, float* DG, float* DCF);
// out[r][c] = (u(r,c) > p) ? 1/(1-p) : 0 with u ~ U[0,1) from a counter-based hash of (seed, element) -- the mask recipe of
// bilstm-parallel-layer.h:54-61 (SetRandUniform / SetRandUniformCol, Add(-p), ApplyHeaviside, Scale(1/(1-p))); per_column
// draws one value per column and repeats it down the rows (SetRandUniformCol, cpucompute/matrix.cc:952-965).
void dropout_mask(hipStream_t st, float* out, long rows, int cols, int ld, float p, unsigned long long seed, bool per_column);
// <Sigmoid> / <Tanh> layers: y = f(x) (cuda-kernels.cu:687-697, 713-727) and d *= f'(y) in place (:699-709, :730-740)
void activation_rows(hipStream_t st, bool tanh_, const float* x, int ldx, float* y, int ldy, long rows, int cols);
void activation_diff_rows(hipStream_t st, bool tanh_, const float* y, int ldy, float* d, int ldd, long rows, int cols);
// out[r][c] = a[r][c] * m[r][c]   (MulElements, :416 / :895)
void mul_elements(hipStream_t st, const float* a, int lda, const float* m, int ldm, float* out, int ldo, long rows, int cols);
// What runs a layer's time recurrence: the whole recurrence in ONE launch per sequence window, with W_m resident in registers
// (lstm_persistent.hip).  ONE selection function per pass (lstm_fwd_plan / lstm_bwd_plan, rec_plan.cpp) decides the instantiation and
// answers every question about it; the launchers execute the plan they are given, and everything else that has to know -- the gating
// and early-middle rules of Net::forward_pass, the buffers and the per-minibatch side-stream rule of Net::backpropagate, the
// exchange-schedule rule of the data-parallel path (comm.cpp), eesen_net_plan_string, the tests -- reads the SAME plan, computed once
// per layer and pass, so a rule cannot drift away from what the launcher runs.  Plans are not kept across minibatches:
// they depend on the minibatch shape, the layer's dropout mode and the buffers reserved so far.
enum { kRecNone = 0, kRecFwdBf = 1, kRecFwdMux = 2, kRecFwdF32 = 3, kRecBwdQ4 = 4, kRecBwdKsplit = 5, kRecBwdKsplitMux = 6, kRecBwdGeneric = 7 };
struct RecPlan {
  int kind = kRecNone;        // kRecNone: no persistent tile fits this shape -- the one-launch-per-step kernels of lstm.hip
  const char* kernel = "";    // the instantiation, e.g. "lstm_bwd_persistent_q4_kernel<8,4>"
  int seq_tile = 0;           // sequences per workgroup
  int units = 0;              // hidden units per workgroup
  int windows = 0;            // launches per layer pass (sequence windows, one after the other)
  int grid[3] = {0, 0, 0};    // (unit blocks, directions, sequence groups) of ONE launch; launched as a 1-D grid of their product
  int wgs = 0;                // workgroups per launch
  int wgs_per_cu = 0;         // ... per CU of this process's share of the device (EESEN_GPU_SHARE)
  int vgprs = 0, lds = 0;     // registers per lane / static LDS bytes of the instantiation (hipFuncGetAttributes = the code object's
                              // .vgpr_count / .group_segment_fixed_size: pinned by tests/test_kernel_resources.py); 0: not known
  int free_vgprs = -1;        // registers per SIMD lane this grid leaves on a CU it occupies: 512 - waves per SIMD x allocated (-1: not known)
  // forward, for consumers of the pass's rows while it runs (net.cpp).  The arrival counters of a gated consumer: grid[0] workgroups
  // per (direction, sequence tile) group of `units` cells each, `seq_tiles` sequence tiles over the whole batch
  int seq_tiles = 1;
  bool one_window = false;    // the whole batch steps together in one launch (not so: sequence windows; the time-multiplexed kernel, whose
                              // one launch steps two sequence tiles in turn; no persistent tile)
  bool leaves_room = false;   // the grid leaves register and LDS room for a 128 x 128 GEMM workgroup on the same CU ("the middle first")
  bool bf16 = false;          // the recurrent product on bf16 operands (eesen_net_set_forward_precision(1) and the shape allows)
  // backward
  bool light = false;         // the 4- / 8-sequence tiles, beside which a side-stream GEMM workgroup keeps a third of its rate
  size_t need_px = 0, need_ex = 0;   // floats of LstmLayerDev::PX (px_floats) and EX the launch must be handed (0: none)
  bool need_dgh = false;             // ... and LstmLayerDev::DGH, [T*S x ndir*4H] words
  // for the launcher
  size_t ctl_words = 0;       // arrival-counter words one launch clears (at most kCtlHalf)
  int chunk = 0;
  const void* fn = nullptr;
  const void* fn_guard = nullptr;   // forward: the same tile with the row guards of LstmLayerDev::guard, where that instantiation exists (launched when a guard is set)
};
RecPlan lstm_fwd_plan(const LstmLayerDev& L);
RecPlan lstm_bwd_plan(const LstmLayerDev& L);
// Execute a plan whose kind is not kRecNone (those shapes take the step kernels above).  cnt: kCtlHalf zero-initialisable counter
// words, err: one word raised when a bounded spin gives up.  after_reset: recorded once the counters are cleared, where the plan is
// one_window (a gated consumer may poll from there on).
void lstm_fwd_launch(hipStream_t st, const RecPlan& plan, const LstmLayerDev& L, unsigned* cnt, unsigned* err, int spin_limit,
                     unsigned long long* trace = nullptr, hipEvent_t after_reset = nullptr);
void lstm_bwd_launch(hipStream_t st, const RecPlan& plan, const LstmLayerDev& L, const float* dY, int lddy, float* DG, unsigned* cnt,
                     unsigned* err, int spin_limit, unsigned long long* trace = nullptr);
// bias_grad[ndir*4H] = column sums of DG; peep_grad[ndir][3][H] = the diag(D^T C) products of
// bilstm-parallel-layer.h:507-510 / :598-601.  ws: >= red_rows_ws(...) floats.
void lstm_bias_peep_grads(hipStream_t st, const LstmLayerDev& L, const float* DG, float* bias_grad, float* peep_grad,
                          float* ws, size_t ws_floats);
size_t lstm_bias_peep_ws_floats(int T, int S, int H, int ndir);

// out[c] = sum_r M[r][c]  (bias gradient of AffineTransform, affine-trans-layer.h:183)
void col_sums(hipStream_t st, const float* M, int rows, int cols, int ld, float* out, float* ws, size_t ws_floats);
size_t col_sums_ws_floats(int rows, int cols);

// ---------------------------------------------------------------------------------------- ctc.hip
// y = softmax(x) per row (Softmax::PropagateFnc, softmax-layer.h:44-47)
void softmax_rows(hipStream_t st, const float* x, int ldx, float* y, int ldy, int rows, int K);
// out = log(in) elementwise on a [rows x K] matrix (CuMatrixBase::ApplyLog, ctc-loss.cc:132-133)
void log_rows(hipStream_t st, const float* in, int ldi, float* out, int ldo, int rows, int K);
// alpha and beta lattice sweeps for all S sequences (2*S workgroups of ctc_sweep_waves(Lpad) wavefronts: one up to Lpad = 256).
// logp: [T*S x K] (ld), labx: [S x Lpad] expanded labels (-1 padded), lens/lablens: [S]
// alpha/beta: [S][T][Lpad] (utterance-major), pzx: [S].  Lpad in {64, 128, ..., 4096}.  waves: 0 = the default for Lpad.
void ctc_alpha_beta(hipStream_t st, const float* logp, int ld, int T, int S, int Lpad, const int* labx, const int* lens,
                    const int* lablens, float* alpha, float* beta, float* pzx, int waves = 0);
int ctc_sweep_waves(int Lpad, int waves = 0);
// Best-path (Viterbi) alignment over the same lattices.  ctc_best_path: the alpha sweep in the max-plus semiring, S workgroups; the
// delta rows are written in alpha's layout [S][T][Lpad] (rows t >= lens[s] are not written).  scores: [T*S x K] (ld) log-domain.
// lattices > 0: that many workgroups instead of S, lattice i of the launch reading the score rows of utterance (lat0 + i) / lpu (labx,
// lens, lablens and delta are indexed by i): the N-best entries of a decode call, lpu = nbest (Ctc::decode_stamps).
void ctc_best_path(hipStream_t st, const float* scores, int ld, int T, int S, int Lpad, const int* labx, const int* lens,
                   const int* lablens, float* delta, int waves = 0, int lattices = 0, int lat0 = 0, int lpu = 1);
// ctc_score: the exact log-score of NL labellings (INTEGRATION.md "Rescoring"): the alpha sweep of ctc_alpha_beta, step for step, that
// stores no row; one workgroup per lattice, all in one launch.  Lattice i (labx [NL][Lpad], lens / lablens / utt [NL]) reads the score
// rows of utterance utt[i] in [0, S); scores [T*S x K] (ld) log-domain, clamped from below at -1e30 as they are read.  score [NL] =
// logadd of the two final cells with the larger as the base; -1e30 where no path exists (and where lablens[i] = 0: no lattice); 0 for
// the one-position lattice of the empty labelling over no frames.
void ctc_score(hipStream_t st, const float* scores, int ld, int T, int S, int NL, int Lpad, const int* labx, const int* lens,
               const int* lablens, const int* utt, float* score, int waves = 0);
// ctc_traceback: from argmax(delta[n-1][L'-1], delta[n-1][L'-2]) (the final blank wins a tie) back to t = 0, the smallest move winning
// among equal predecessors.  ali / pos [T*S] (row t*S + s): class id / lattice position per frame, -1 on rows t >= lens[s] and on
// every row of an utterance without a feasible path; score [S]: the path's log-score, -1e30 without one.
void ctc_traceback(hipStream_t st, const float* delta, int T, int S, int Lpad, const int* labx, const int* lens, const int* lablens,
                   int* ali, int* pos, float* score);
// ctc_stamp: label intervals out of the positions of NL best paths (INTEGRATION.md "Time stamps and CTM").  pos: ctc_traceback's
// output of the lattices in groups of G (the last may be smaller), group g as [T][lattices of g] at offset g * G * T; lens [NL].
// lstart / lend [NL][T]: first frame of label u and one past its last, -1 beyond the labels and without a path.
void ctc_stamp(hipStream_t st, const int* pos, int T, int NL, int G, const int* lens, int* lstart, int* lend);
// ctc_hyp_lattices (ctc_decode.hip): the expanded labels of the NL = S * N hypotheses ctc_hyp / ctc_word_hyp left, for the sweeps above.
// labx [NL][Lpad] blank-interleaved, -1 padded; lablens [NL] = 2 U + 1; lat_lens [NL] = the utterance's frames, or 0 -- no lattice --
// for the empty hypothesis, for one of more labels than (Lpad - 1) / 2 and for ranks beyond the returned count (hyp_len < 0).
// utt != null: the lattices of ctc_score instead -- the empty hypothesis gets its one-position lattice (lablens 1) and its utterance's
// frames, an entry without a lattice lablens = 0 and no frames, and utt [NL] = i / N, the utterance whose score rows lattice i reads.
void ctc_hyp_lattices(hipStream_t st, const int* hyp, const int* hyp_len, const int* lens, int T, int NL, int N, int Lpad, int* labx,
                      int* lablens, int* lat_lens, int* utt = nullptr);
// edit_distance_jobs (edit_distance.hip): batched Levenshtein distance, unit costs, the total only -- edit_distance() of ctc_host.cpp,
// integer for integer.  jobs [njobs][4] = (offset a, length a, offset b, length b), a into tok_a, b into tok_b; out [njobs].  One wavefront per job, all in
// one launch.  max_len: the longest sequence any job names (<= kEditDistanceMaxLen), which sizes the boundary column in LDS.
constexpr int kEditDistanceMaxLen = 8192;
void edit_distance_jobs(hipStream_t st, const int* tok_a, const int* tok_b, const int* jobs, int njobs, int max_len, int* out);
// Prefix beam search, lexicon-free or along a lexicon trie (ctc_decode.hip; the computation: INTEGRATION.md "Decoding").  scores: [T*S x K] (ld) log-domain.
// ctc_row_topc: per row t*S + s with t < lens[s] the Cc = min(max_classes, K - 1) best non-blank classes -- ids ascending in
// cid [rows][Cc], their scores in csc [rows][Cc], the blank's in sblank [rows]; every score clamped from below at -1e30.
void ctc_row_topc(hipStream_t st, const float* scores, int ld, int rows, int K, int S, const int* lens, int Cc, int* cid, float* csc,
                  float* sblank);
struct LmTables;
struct LexTables;
// ctc_prefix_beam: S workgroups, each walks its utterance's frames.  tparent / tlabel [S][1 + T*B]: the trie (node 0 = the empty
// prefix), written only; fnode / flen / fscore [S][B]: node, length and total of the final beam, best first (-1, -1, -1e30 beyond
// count[s] live entries).  1 <= B <= 64, 1 <= Cc <= 64, B * Cc <= 2048.  lm == lex == null: the plain search (ctc_prefix_beam_kernel
// <false>; alpha, beta, use_eos and flm are not read).  lm alone: the same search with a token n-gram LM fused in (<true>; INTEGRATION.md
// "LM fusion"; the tables: lm.h): an extension by class c adds g = alpha * w + beta, (w, next) = lm_step(the entry's LM state, c);
// with use_eos, alpha * fin[state] joins every total after the last frame and the final beam is re-ranked.  flm [S][B]: the
// unweighted LM sum of each final entry.  lex: extensions only along the lexicon trie (ctc_prefix_beam_lex_kernel; INTEGRATION.md "Lexicon"; the
// tables: lex.h); lm is then a model over word ids, stepped once per closed word, or null; beta is per word; the final beam holds
// only the entries that end on a word end, and count[s] counts those.  la (device, [lexicon nodes], or null; needs lex and lm): the
// unigram look-ahead (ctc_prefix_beam_lex_la_kernel; INTEGRATION.md "LM look-ahead"): candidates are ranked by total + alpha * la[node] + beta;
// la_edge [edges]: la of every edge's target, la_edge[e] = la[child_node[e]].
void ctc_prefix_beam(hipStream_t st, const float* scores, int ld, int T, int S, const int* lens, int B, int Cc, const int* cid,
                     const float* csc, const float* sblank, const LmTables* lm, const LexTables* lex, const float* la, const float* la_edge,
                     float alpha, float beta, bool use_eos, int* tparent, int* tlabel, int* fnode, int* flen, float* fscore, float* flm, int* count);
// ctc_hyp: hyp [S][N][T] the labels of the N best entries front to back (-1 beyond the length), hyp_len / score [S][N] (-1 / -1e30
// beyond count[s]); with flm and lm_out (both null without an LM) lm_out [S][N] = flm of the same entries, -1e30 beyond count[s].
void ctc_hyp(hipStream_t st, const int* tparent, const int* tlabel, const int* fnode, const int* flen, const float* fscore, const float* flm,
             const int* count, int T, int S, int B, int N, int* hyp, int* hyp_len, float* score, float* lm_out);
// ctc_word_beam: the word beam search along an unspaced lexicon (ctc_word_beam_kernel; INTEGRATION.md "Words without a boundary
// unit"; the tables: lex.h), S workgroups as ctc_prefix_beam.  The trie gains tword [S][1 + T*B]: the word closed in front of a
// node's label, or 0.  Final hypotheses, best first, [S][B]: fnode, flen (labels), fscore, flm, fword (the word closed at the end, 0
// for the empty hypothesis), fnw (words, the last included); count[s] of them.  B * (1 + Cc * (1 + lex->H)) <= 4096.
struct WordLexTables;
void ctc_word_beam(hipStream_t st, const float* scores, int ld, int T, int S, const int* lens, int B, int Cc, const int* cid,
                   const float* csc, const float* sblank, const LmTables* lm, const WordLexTables& lex, const float* la /*or null: as above*/,
                   float alpha, float beta, bool use_eos, int* tparent, int* tlabel, int* tword, int* fnode, int* flen, float* fscore, float* flm, int* fword, int* fnw, int* count);
// ctc_word_hyp: ctc_hyp's outputs plus words / ends [S][N][T] (word ids front to back and the number of labels up to and including
// each word's last; -1 beyond the word count) and word_len [S][N] (-1 beyond count[s]).
void ctc_word_hyp(hipStream_t st, const int* tparent, const int* tlabel, const int* tword, const int* fnode, const int* flen, const float* fscore,
                  const float* flm, const int* fword, const int* fnw, const int* count, int T, int S, int B, int N, int* hyp, int* hyp_len,
                  float* score, float* lm_out, int* words, int* ends, int* word_len);
// diff[t*S+s][k] = y*rowsum(e) - gamma ... (error kernel + softmax Jacobian, ctc-loss.cc:156-168)
// labx [S x Lpad]: the expanded labels (blank 0 at even positions), lablens [S] = 2 U_s + 1
void ctc_error_diff(hipStream_t st, const float* probs, int ld, int T, int S, int K, int Lpad, int Lmax, const int* lens,
                    const int* lablens, const int* labx, const float* alpha, const float* beta,
                    const float* pzx, float* diff, int ldd);
// in place: m = (apply_log ? log m : m) - prior_scale * log_prior[col]; log_prior may be null (net-output-extract.cc:103-112)
void log_sub_prior(hipStream_t st, float* m, int ld, int rows, int K, bool apply_log, const float* log_prior, float prior_scale);
// ids[r] = argmax_k m[r][k], first maximum wins (CuMatrixBase::FindRowMaxId, cuda-matrix.cc:1038-1095)
void row_argmax(hipStream_t st, const float* m, int ld, int rows, int K, int* ids);

// ---------------------------------------------------------------------------------------- ce.hip
// CE::EvalParallel (ce-loss.cc:94-169) in one pass over the softmax outputs y [rows x K] (row t*S + s valid iff t < lens[s]):
// diff = (y - onehot(tgt)) * mask (padded rows 0), and into *out the sums over valid rows of -log y[tgt] and of
// [argmax(y) == tgt] (row_argmax's tie rule), reduced in a fixed order through `part` (ce_eval_blocks(rows) entries).
struct CeSums {
  double obj;
  long long correct;
};
int ce_eval_blocks(int rows);
void ce_eval(hipStream_t st, const float* y, int ld, int rows, int K, int S, const int* lens, const int* tgt, float* diff,
             int ldd, CeSums* part, CeSums* out);

// ---------------------------------------------------------------------------------------- optim.hip
// corr = mmt*corr + fresh; clip to +-max_grad when max_grad > 0; param -= lr_coef*corr
// skip (may be null): device word; when non-zero at execution time the update is a no-op (see optim.hip)
// live (may be null): device float; when ZERO at execution time the update is a no-op (data-parallel closing round, comm.cpp)
void sgd_update(hipStream_t st, float* param, float* corr, const float* fresh, long n, float mmt, float lr_coef,
                float max_grad, const unsigned* skip = nullptr, const float* live = nullptr);
// p[0..n) = 0 when *word != 0 at execution time (the recurrence kernels' error word): see optim.hip / comm.cpp
void zero_if_set(hipStream_t st, float* p, long n, const unsigned* word);
// Adagrad (rmsprop = false) / RMSProp update of one flat parameter block, see optim.hip
void adaptive_update(hipStream_t st, float* param, float* corr, const float* fresh, float* accu, long n, float mmt, float lr,
                     float max_grad, float eps, float rho, float one_minus_rho, bool rmsprop, const unsigned* skip = nullptr,
                     const float* live = nullptr);
// Moments of a [rows x cols] region (leading dimension ld) of a flat buffer, as MomentStatistics prints them
// (/root/reference/src/net/utils-functions.h:50-82): out6 = {min, max, mean, variance, skewness, kurtosis}, doubles on the
// device; two passes (min / max / sum, then the central power sums), fp64 accumulation.  ws: >= 8 doubles of scratch.
void tensor_moments(hipStream_t st, const float* base, long rows, int cols, long ld, double* out6, double* ws,
                    int nb = 0, int hf = 0, int hi = 0);   // (nb, hf, hi): column c of the tensor lives at (c / hf) * hi + c % hf of its row (0: at c)
// dst[c][r] = src[r][c]  (rows x cols -> cols x rows), dense
void transpose2d(hipStream_t st, const float* src, int rows, int cols, float* dst);
// dst[r][0..cols) = src[r][0..cols) with different leading dimensions
void copy2d(hipStream_t st, const float* src, int lds, float* dst, int ldd, int rows, int cols);

}  // namespace eesen
