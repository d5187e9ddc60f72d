// feeder.hip -- minibatch assembly on the device, double-buffered (row a1 of the hot-path table).
//
// The reference builds every minibatch on the host: a zeroed host matrix of max_frame_num * S rows, one row copy per frame
// into row t*S + s (/root/reference/src/netbin/train-ctc-parallel.cc:186-193), then a blocking host-to-device copy of
// the PADDED matrix (:195 `feats_transf = feat_mat_host`).  Here the host only packs the S utterance matrices back to back
// into a pinned staging slot (no padding crosses PCIe); the copy runs on the feeder's own stream and a kernel writes the
// zero-padded, time-major interleaved matrix in HBM.  Slots rotate, so the staging of batch n+1 overlaps the training
// step of batch n; the compute stream only waits for the slot's event.
//
// The interleave is pure byte movement (HBM-bound, a few MB per batch): one thread per output float4 (or float when
// D % 4 != 0), reads coalesced along d within a frame, writes fully coalesced; padded frames are written as zeros by the
// same kernel, so the output needs no memset.
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "cmvn_stats.h"
#include "fbank.h"
#include "guard.h"
#include "pitch.h"

namespace eesen {
namespace {

template <int V>  // V = floats per thread (4: D % 4 == 0 and 16-byte aligned rows, else 1)
__global__ __launch_bounds__(256) void interleave_kernel(const float* __restrict__ packed, const long* __restrict__ off,
                                                        const int* __restrict__ frames, float* __restrict__ out, int T,
                                                        int S, int D, int ld) {
  const int dv = D / V;
  const long n = (long)T * S * dv;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int d = (int)(i % dv) * V;
    const long r = i / dv;  // output row t*S + s
    const int s = (int)(r % S), t = (int)(r / S);
    float* dst = out + r * ld + d;
    if (V == 4) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (t < frames[s]) v = *reinterpret_cast<const float4*>(packed + off[s] + (long)t * D + d);
      *reinterpret_cast<float4*>(dst) = v;
    } else {
      *dst = t < frames[s] ? packed[off[s] + (long)t * D + d] : 0.f;
    }
  }
}

// ---- feature front end ----------------------------------------------------------------------------------------------------
// The recipes feed the trainer through a pipe of host filters, e.g. (asr_egs/wsj/steps/train_ctc_parallel.sh:95-110,
// decode_ctc_lat.sh:92-95, librispeech/steps/train_ctc_parallel_mult.sh:110-133)
//   apply-cmvn --norm-vars=true --utt2spk=ark:utt2spk scp:cmvn.scp scp:train.scp ark:- | splice-feats --left-context=1
//   --right-context=1 ark:- ark:- | subsample-feats --n=3 --offset=0 ark:- ark:- | add-deltas ark:- ark:- |
// Every one of these is a per-dimension affine map or a clamped row gather -- bytes, not arithmetic -- so they run here, on
// the packed utterance matrices in HBM between the PCIe copy and the interleave: the raw features cross PCIe once (three
// times fewer bytes than with deltas applied on the host) and no host filter processes sit in front of a GPU that consumes
// hundreds of thousands of frames per second.  One launch per stage, one thread per output element, utterance = blockIdx.y.
// Arithmetic is the reference's, operation for operation and WITHOUT fused multiply-add, so the results equal a scalar
// host evaluation bit for bit (the reference's own AddVec goes through BLAS saxpy, whose rounding depends on the BLAS build).
struct StageDev { int kind, a, b; };

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__global__ __launch_bounds__(256) void feat_stage_kernel(StageDev st, const float* __restrict__ scales, const float* __restrict__ src,
                                                        const long* __restrict__ off_in, const int* __restrict__ fr_in, int Din,
                                                        float* __restrict__ dst, const long* __restrict__ off_out,
                                                        const int* __restrict__ fr_out, int Dout, const float* __restrict__ cmvn) {
#pragma clang fp contract(off)   // hipcc contracts a * b + c into one fma by default; __fmul_rn / __fadd_rn do not help (header inlines built with that default)
  // the delta windows (at most 9 orders x 33-wide steps: 1161 floats) sit in LDS: the tap loop then has no dependent global load
  // in front of every tap, and the taps' feature loads are independent of each other
  __shared__ float s_sc[1200];
  if (st.kind == EESEN_FEAT_DELTAS) {
    const int nsc = (st.a + 1) + st.b * st.a * (st.a + 1);
    for (int i = threadIdx.x; i < nsc; i += blockDim.x) s_sc[i] = scales[i];
    __syncthreads();
  }
  const int s = blockIdx.y;
  const int Ti = fr_in[s], To = fr_out[s];
  const float* x = src + off_in[s];
  float* y = dst + off_out[s];
  const long n = (long)To * Dout;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int t = (int)(i / Dout), c = (int)(i % Dout);
    float v;
    if (st.kind == EESEN_FEAT_CMVN) {                      // feat/cmvn.cc:112-116: f = norm(0, d) + f * norm(1, d)
      const float* nm = cmvn + (size_t)s * 2 * Din;
      const float prod = x[(long)t * Din + c] * nm[Din + c];
      v = nm[c] + prod;
    } else if (st.kind == EESEN_FEAT_SPLICE) {             // feat/feature-functions.cc:401-411
      const int j = c / Din, d = c % Din;
      v = x[(long)clampi(t + j - st.a, Ti - 1) * Din + d];
    } else if (st.kind == EESEN_FEAT_SUBSAMPLE) {          // featbin/subsample-feats.cc:93-108
      const int ti = st.a > 0 ? st.b + st.a * t : t / (-st.a);
      v = x[(long)ti * Din + c];
    } else {                                               // DeltaFeatures::Process, feat/feature-functions.cc:252-266
      const int o = c / Din, d = c % Din;
      const int max_off = o * st.b;
      const float* sc = s_sc + o + st.b * o * (o - 1);     // windows of orders 0..o-1 hold 1 + 2kW entries each
      v = 0.f;
      for (int j = -max_off; j <= max_off; ++j) {
        const float w = sc[j + max_off];
        const float prod = w * x[(long)clampi(t + j, Ti - 1) * Din + d];
        v = w != 0.f ? v + prod : v;                         // a zero tap is SKIPPED by the reference (:263), not added
      }
    }
    y[i] = v;
  }
}

// paste-feats (src/featbin/paste-feats.cc:56-63): utterance s of the output is [fr_out[s] x Dout], its row t the rows t of the 2..4
// inputs side by side.  The inputs are ragged matrices packed back to back, each with its own width and per-utterance offsets, and
// may hold MORE rows than the output (the join trims to the shortest).  One output element per thread, utterance = blockIdx.y, plain
// float loads and stores: rows are 43 or 83 floats wide, so neither side is 16-byte aligned from one row to the next; consecutive
// threads still write consecutive floats and read runs of dim[j] consecutive floats.  A dropped utterance has fr_out[s] = 0 and is
// left alone.
constexpr int kPasteMaxInputs = 4;
struct PasteArgs {
  const float* src[kPasteMaxInputs];
  const long* off[kPasteMaxInputs];    // off[j][s]: floats in front of utterance s in input j
  int dim[kPasteMaxInputs], start[kPasteMaxInputs];   // width of input j and its first output column
  int n;
};

__global__ __launch_bounds__(256) void feat_paste_kernel(PasteArgs a, float* __restrict__ dst, const long* __restrict__ off_out,
                                                        const int* __restrict__ fr_out, int Dout) {
  const int s = blockIdx.y;
  const long n = (long)fr_out[s] * Dout;
  if (n == 0) return;
  const float* x[kPasteMaxInputs];
#pragma unroll
  for (int j = 0; j < kPasteMaxInputs; ++j) x[j] = j < a.n ? a.src[j] + a.off[j][s] : nullptr;
  float* y = dst + off_out[s];
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long t = i / Dout;
    const int c = (int)(i - t * Dout);
    const float* p = x[0];
    int d = a.dim[0], c0 = 0;
#pragma unroll
    for (int j = 1; j < kPasteMaxInputs; ++j)
      if (j < a.n && c >= a.start[j]) { p = x[j]; d = a.dim[j]; c0 = a.start[j]; }
    y[i] = p[t * d + (c - c0)];
  }
}

// the grid of a launch with utterance = blockIdx.y over an output whose largest utterance holds `biggest` floats: one element per
// thread (a stage is latency-bound otherwise), at most 2048 blocks along x
dim3 stage_grid(long biggest, int S) { return dim3((unsigned)std::min<long>(std::max<long>(cdivl(biggest, 256), 1), 2048), S); }

void paste_launch(PasteArgs a, float* dst, const long* off_out, const int* fr_out, int Dout, int S, long biggest, hipStream_t st) {
  a.start[0] = 0;
  for (int j = 1; j < kPasteMaxInputs; ++j) a.start[j] = j < a.n ? a.start[j - 1] + a.dim[j - 1] : 0;
  hipLaunchKernelGGL(feat_paste_kernel, dim3(stage_grid(biggest, S)), dim3(256), 0, st, a, dst, off_out, fr_out, Dout);
  check_launch("feat_paste_kernel");
}

// DeltaFeatures::DeltaFeatures, feat/feature-functions.cc:216-241, in the reference's float arithmetic
std::vector<float> delta_scales(int order, int window) {
  std::vector<std::vector<float>> sc(order + 1);
  sc[0] = {1.0f};
  for (int i = 1; i <= order; ++i) {
    const std::vector<float>& prev = sc[i - 1];
    std::vector<float>& cur = sc[i];
    const int prev_offset = ((int)prev.size() - 1) / 2, cur_offset = prev_offset + window;
    cur.assign(prev.size() + 2 * window, 0.f);
    float normalizer = 0.0f;
    for (int j = -window; j <= window; ++j) {
      normalizer += j * j;
      for (int k = -prev_offset; k <= prev_offset; ++k) cur[j + k + cur_offset] += static_cast<float>(j) * prev[k + prev_offset];
    }
    const float alpha = (float)(1.0 / normalizer);           // VectorBase<float>::Scale(1.0 / normalizer)
    for (float& v : cur) v *= alpha;
  }
  std::vector<float> flat;
  for (const auto& v : sc) flat.insert(flat.end(), v.begin(), v.end());
  return flat;
}

}  // namespace

struct Feeder {
  struct Slot {
    // Pinned staging, owned only: its reuse is ordered by `ready` (the slot's copies and kernels have run), not by a use of its own.
    PinBuf host;            // the utterance matrices back to back
    PinBuf tab_h;           // the batch's tables (BatchTables, feat_layout.h): one block here, one on the device, one upload
    DevBuf<long> tab_d;
    DevBuf<float> packed, out;
    DevEvent ready, consumed;
    bool in_flight = false, has_consumer = false;
    int T = 0, S = 0, D = 0, ld = 0;
    // feature front end: the second packed buffer of the stage ping-pong, the CMVN vectors
    DevBuf<float> packed2, cmvn_d;
    PinBuf cmvn_h;
    // filterbank + pitch head stage: the filterbank matrix before the join, and the pitch tracker's scratch
    DevBuf<float> fbank;
    PitchScratch pitch;
    // the statistics tap: the chunks' partial sums, the batch's statistics, and their pinned copy (read after `ready`)
    DevBuf<double> stats_part, stats_d;
    PinBuf stats_h;
    int stats_D = 0;        // the dimension at the tapped boundary; 0: this batch was not tapped
  };
  struct Stage { int kind, a, b; size_t scale_off; };
  std::vector<Stage> pipe;
  int tap = -1;             // the stage boundary whose CMVN statistics are computed beside the assembly (-1: none)
  std::vector<long> tab;    // a batch's tables while it can still be refused: no slot is taken before they are complete
  DevBuf<float> scales_d;
  // EESEN_FEAT_FBANK, the head stage that turns waveforms into features (fbank.hip); every waveform submitted gets a dither key of its own
  std::unique_ptr<FbankPlan> fb_plan;
  FbankDev fb_dev;
  unsigned long long fb_next_id = 0;
  // EESEN_FEAT_FBANK_PITCH adds the pitch tracker (pitch.hip) beside it; a waveform's key is the same for the dither and the delta-pitch noise
  std::unique_ptr<PitchPlan> pt_plan;
  PitchDev pt_dev;
  int device;
  hipStream_t compute;
  DevStream copy;
  std::vector<Slot> slots;
  int next = 0;

  Feeder(int dev, void* compute_stream, int nslots) : device(dev), compute(static_cast<hipStream_t>(compute_stream)) {
    EESEN_REQUIRE(nslots >= 1 && nslots <= 8, EESEN_ERR_INVALID, "1..8 staging slots");
    require_device(dev);
    EESEN_HIP_CHECK(hipStreamCreateWithFlags(&copy.s, hipStreamNonBlocking));
    slots.resize(nslots);
  }
  ~Feeder() {   // drained here; the slots and the copy stream go with the members
    (void)hipSetDevice(device);
    if (copy) (void)hipStreamSynchronize(copy);
  }
  // the slot's previous batch: its copy + kernels must have run (the pinned staging is overwritten) and its consumer must have
  // finished reading the assembled matrix (`out` is overwritten)
  Slot& next_slot(int* id) {
    *id = next;
    next = (next + 1) % (int)slots.size();
    Slot& sl = slots[*id];
    if (sl.in_flight) sl.ready.wait();
    if (sl.has_consumer) sl.consumed.wait();
    sl.in_flight = sl.has_consumer = false;
    return sl;
  }
  void drain() {   // batches in flight still read the tables a set_* call is about to replace
    for (auto& s : slots)
      if (s.in_flight) s.ready.wait();
  }
  // the raw matrices back to back in the slot's pinned staging (a quarter more when it has to grow), rows made contiguous
  static float* pack(Slot& sl, const float* const* utts, const int* frames, const int* strides, const long* off, int S, int D, long total) {
    float* host = static_cast<float*>(sl.host.reserve((size_t)total * sizeof(float), ((size_t)total + (size_t)total / 4) * sizeof(float)));
    for (int s = 0; s < S; ++s) {
      const int st = strides ? strides[s] : D;
      if (st == D) std::memcpy(host + off[s], utts[s], (size_t)frames[s] * D * sizeof(float));
      else for (int t = 0; t < frames[s]; ++t) std::memcpy(host + off[s] + (long)t * D, utts[s] + (long)t * st, (size_t)D * sizeof(float));
    }
    return host;
  }

  // ---- feature front end (see feat_stage_kernel) ----
  void set_pipeline(const eesen_feat_stage_t* st, int n) {
    EESEN_REQUIRE(n >= 0 && n <= 8, EESEN_ERR_INVALID, "0..8 front-end stages");
    EESEN_HIP_CHECK(hipSetDevice(device));
    std::vector<Stage> np;
    std::vector<float> scales;
    int n_cmvn = 0;
    for (int k = 0; k < n; ++k) {
      Stage g{st[k].kind, st[k].a, st[k].b, 0};
      switch (g.kind) {
        case EESEN_FEAT_FBANK:
          EESEN_REQUIRE(k == 0, EESEN_ERR_INVALID, "the filterbank stage reads waveforms: it must be the first stage");
          EESEN_REQUIRE(fb_plan != nullptr, EESEN_ERR_STATE, "the filterbank stage needs its options first (eesen_feeder_set_fbank)");
          break;
        case EESEN_FEAT_FBANK_PITCH:
          EESEN_REQUIRE(k == 0, EESEN_ERR_INVALID, "the filterbank + pitch stage reads waveforms: it must be the first stage");
          EESEN_REQUIRE(fb_plan != nullptr, EESEN_ERR_STATE, "the filterbank + pitch stage needs the filterbank options first (eesen_feeder_set_fbank)");
          EESEN_REQUIRE(pt_plan != nullptr, EESEN_ERR_STATE, "the filterbank + pitch stage needs the pitch options first (eesen_feeder_set_pitch)");
          require_same_rate();
          EESEN_REQUIRE(g.a >= 0, EESEN_ERR_INVALID, "paste-feats: --length-tolerance must not be negative");
          break;
        case EESEN_FEAT_CMVN: ++n_cmvn; break;
        case EESEN_FEAT_SPLICE:   // KALDI_ASSERT(left_context >= 0 && right_context >= 0), feature-functions.cc:398
          EESEN_REQUIRE(g.a >= 0 && g.b >= 0 && g.a + g.b <= 64, EESEN_ERR_INVALID, "splice-feats: context must be 0..64 frames");
          break;
        case EESEN_FEAT_SUBSAMPLE:  // subsample-feats.cc:52-55
          EESEN_REQUIRE(g.a != 0, EESEN_ERR_INVALID, "subsample-feats: n must not be 0");
          EESEN_REQUIRE(g.a > 0 ? g.b >= 0 : g.b == 0, EESEN_ERR_INVALID, "subsample-feats: --offset cannot be used with negative n (and must be >= 0)");
          break;
        case EESEN_FEAT_DELTAS: {  // feature-functions.cc:211-213
          EESEN_REQUIRE(g.a >= 0 && g.a <= 8 && g.b > 0 && g.b <= 16, EESEN_ERR_INVALID, "add-deltas: order 0..8, window 1..16");
          g.scale_off = scales.size();
          const std::vector<float> sc = delta_scales(g.a, g.b);
          scales.insert(scales.end(), sc.begin(), sc.end());
          break;
        }
        default: throw Error(EESEN_ERR_INVALID, "unknown front-end stage kind " + std::to_string(g.kind));
      }
      np.push_back(g);
    }
    EESEN_REQUIRE(n_cmvn <= 1, EESEN_ERR_INVALID, "at most one CMVN stage");
    EESEN_REQUIRE(tap <= n, EESEN_ERR_INVALID, "the statistics tap sits on boundary " + std::to_string(tap) + ", beyond this pipeline: move it first (eesen_feeder_set_stats_tap)");
    drain();
    if (!scales.empty()) {
      scales_d.reserve(scales.size());
      EESEN_HIP_CHECK(hipMemcpy(scales_d.p, scales.data(), scales.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    pipe.swap(np);
  }
  void set_stats_tap(int boundary) {
    EESEN_REQUIRE(boundary >= -1 && boundary <= (int)pipe.size(), EESEN_ERR_INVALID,
                  "the statistics tap goes on boundary 0.." + std::to_string(pipe.size()) + " of the current pipeline, or -1 for none");
    EESEN_HIP_CHECK(hipSetDevice(device));
    drain();
    tap = boundary;
  }
  // AccCmvnStats of every utterance at boundary b, as it lies packed in `x` (unread where the boundary holds no frame), into the slot's
  // pinned block: enqueued on the copy stream behind whatever wrote the boundary
  void tap_stats(Slot& sl, const std::vector<int>& dims, const BatchTables& t, const BatchTables& d, const long* total, int b, int S, const float* x) {
    const int D = dims[b];
    const size_t n = (size_t)S * 2 * (D + 1);
    int longest = 0;
    for (int s = 0; s < S; ++s) longest = std::max(longest, t.frames[(size_t)b * S + s]);
    const int rows = cmvn_chunk_rows(D);
    sl.stats_part.reserve(cmvn_partial_doubles(total[b] / D, S, D, rows));
    sl.stats_d.reserve(n);
    double* h = static_cast<double*>(sl.stats_h.reserve(n * sizeof(double)));
    cmvn_stats_launch(x, d.off + (size_t)b * S, d.frames + (size_t)b * S, nullptr, S, D, longest, rows, sl.stats_part.p, sl.stats_d.p, copy);
    EESEN_HIP_CHECK(hipMemcpyAsync(h, sl.stats_d.p, n * sizeof(double), hipMemcpyDeviceToHost, copy));
    sl.stats_D = D;
  }
  void set_fbank(const eesen_fbank_opts_t& o) {
    std::unique_ptr<FbankPlan> np(new FbankPlan(o));
    EESEN_HIP_CHECK(hipSetDevice(device));
    drain();
    fb_dev.upload(*np);
    fb_plan.swap(np);
  }
  void set_pitch(const eesen_pitch_opts_t& o) {
    std::unique_ptr<PitchPlan> np(new PitchPlan(o));
    EESEN_HIP_CHECK(hipSetDevice(device));
    drain();
    pt_dev.upload(*np);
    pt_plan.swap(np);
  }
  void require_same_rate() const {
    EESEN_REQUIRE(fb_plan->opts.samp_freq == pt_plan->opts.samp_freq, EESEN_ERR_INVALID,
                  "the filterbank + pitch stage reads one waveform: the two --sample-frequency values differ (" +
                      std::to_string(fb_plan->opts.samp_freq) + " vs. " + std::to_string(pt_plan->opts.samp_freq) + ")");
  }
  // rows of the processed pitch matrix of a waveform: frames + delay, none without a frame
  int pitch_rows(int nsamp) const {
    const int f = pt_plan->num_frames(nsamp);
    return f ? f + pt_plan->opts.delay : 0;
  }
  int stage_dim(const Stage& g, int D) const {
    if (g.kind == EESEN_FEAT_FBANK_PITCH) {
      EESEN_REQUIRE(D == 1, EESEN_ERR_INVALID, "the filterbank + pitch stage takes waveforms as [samples x 1] matrices");
      return fb_plan->dim + pt_plan->proc_dim;
    }
    if (g.kind == EESEN_FEAT_FBANK) {
      EESEN_REQUIRE(D == 1, EESEN_ERR_INVALID, "the filterbank stage takes waveforms as [samples x 1] matrices");
      return fb_plan->dim;
    }
    if (g.kind == EESEN_FEAT_SPLICE) return D * (1 + g.a + g.b);
    if (g.kind == EESEN_FEAT_DELTAS) return D * (1 + g.a);
    return D;
  }
  int stage_frames(const Stage& g, int T) const {
    if (g.kind == EESEN_FEAT_FBANK) return fb_plan->num_frames(T);
    if (g.kind == EESEN_FEAT_FBANK_PITCH) {
      const int fr[2] = {fb_plan->num_frames(T), pitch_rows(T)};
      return paste_frames(fr, 2, g.a);
    }
    return g.kind == EESEN_FEAT_SUBSAMPLE ? subsample_frames(T, g.a, g.b) : T;
  }
  int pipeline_dim(int D) const { for (const Stage& g : pipe) D = stage_dim(g, D); return D; }
  int pipeline_frames(int T) const { for (const Stage& g : pipe) T = stage_frames(g, T); return T; }

  // What the head stage of a batch needs beyond its tables: the totals of the two layouts.
  struct Head { int kind = kHeadNone; FbankTotals fb; PitchTotals pt; };

  // The head stage over the slot's samples (boundary 0, already on their way): the filterbank alone writes boundary 1; with the pitch
  // tracker beside it the filterbank writes its scratch matrix, the tracker its own, and the join writes boundary 1.  Everything is
  // enqueued on the copy stream and reads the batch's tables from the slot's device block (`d`).
  void head_stage(Slot& sl, const Head& h, const BatchTables& d, int S, const float* wave, float* dst, int Dout, long biggest) {
    float* fb_out = dst;
    if (h.kind == kHeadFbankPitch) {
      sl.fbank.reserve((size_t)std::max(h.fb.out, 1L));
      fb_out = sl.fbank.p;
    }
    fbank_launch(*fb_plan, fb_dev, wave, d.off, d.frames, d.prefix, d.ids, S, h.fb.frames, fb_out, d.fb_off, copy);
    if (h.kind != kHeadFbankPitch) return;
    pitch_track_launch(*pt_plan, pt_dev, sl.pitch.reserve(*pt_plan, h.pt, S, d.utt, wave), true, copy);
    PasteArgs pa = PasteArgs();
    pa.n = 2;
    pa.src[0] = sl.fbank.p; pa.off[0] = d.fb_off; pa.dim[0] = fb_plan->dim;
    pa.src[1] = sl.pitch.proc.p; pa.off[1] = d.proc_off; pa.dim[1] = pt_plan->proc_dim;
    paste_launch(pa, dst, d.off + S, d.frames + S, Dout, S, biggest, copy);
  }

  // the zero-padded, time-major matrix of the slot from the packed utterances of the last boundary
  void assemble(Slot& sl, const float* packed, const long* off, const int* frames, int T, int S, int D) {
    const int ld = (D + 3) / 4 * 4;  // rows of the assembled matrix start on 16 bytes (GEMM operand alignment)
    const bool fresh = sl.out.reserve((size_t)T * S * ld);
    if (ld != D)  // pad columns stay zero
      EESEN_HIP_CHECK(hipMemsetAsync(sl.out.p, 0, (fresh ? sl.out.cap : (size_t)T * S * ld) * sizeof(float), copy));
    const bool vec = D % 4 == 0;  // then every packed frame and every output row is 16-byte aligned
    const long n = (long)T * S * (vec ? D / 4 : D);
    const int blocks = (int)std::min<long>(cdivl(n, 256), 256L * 32);
    if (vec) interleave_kernel<4><<<blocks, 256, 0, copy>>>(packed, off, frames, sl.out.p, T, S, D, ld);
    else interleave_kernel<1><<<blocks, 256, 0, copy>>>(packed, off, frames, sl.out.p, T, S, D, ld);
    check_launch("interleave_kernel");
    sl.T = T; sl.S = S; sl.D = D; sl.ld = ld;
  }

  // One batch through the stages `pl` (none: the matrices as they are).  Two passes.  The first lays the batch out in `tab` and
  // holds every refusal: it reads counts and compares pointers, takes no slot, waits for nothing and hands out no noise key.  The
  // second takes the slot, packs, uploads (the payload and the tables: two copies) and enqueues the kernels; nothing synchronises.
  int stage_batch(const std::vector<Stage>& pl, const float* const* utts, const int* frames, const int* strides, const float* const* cmvn, int S, int D) {
    EESEN_REQUIRE(S > 0 && D > 0, EESEN_ERR_INVALID, "need at least one utterance and one feature column");
    const int nst = (int)pl.size(), nb = nst + 1;
    std::vector<int> dims(nb);
    dims[0] = D;
    int Dc = 0;   // the feature dimension in front of the CMVN stage (0: no such stage)
    for (int k = 0; k < nst; ++k) {
      if (pl[k].kind == EESEN_FEAT_CMVN) Dc = dims[k];
      dims[k + 1] = stage_dim(pl[k], dims[k]);
    }
    EESEN_REQUIRE(!Dc || cmvn, EESEN_ERR_INVALID, "the pipeline has a CMVN stage: per-utterance offset/scale vectors are required");
    Head h;
    if (nst) h.kind = pl[0].kind == EESEN_FEAT_FBANK ? kHeadFbank : pl[0].kind == EESEN_FEAT_FBANK_PITCH ? kHeadFbankPitch : kHeadNone;
    tab.resize(batch_words(nb, S, h.kind));
    const BatchTables t = batch_carve(tab.data(), nb, S, h.kind);
    std::vector<long> total(nb);
    const int T = boundary_layout(frames, S, dims.data(), nb, [&](int k, int f) { return stage_frames(pl[k], f); }, t.off, t.frames, total.data());
    for (int s = 0; s < S; ++s) {
      EESEN_REQUIRE(frames[s] == 0 || utts[s] != nullptr, EESEN_ERR_INVALID, "null utterance matrix");
      EESEN_REQUIRE(!strides || frames[s] == 0 || strides[s] >= D, EESEN_ERR_INVALID, "row stride smaller than the feature dimension");
      EESEN_REQUIRE(!Dc || frames[s] == 0 || cmvn[s] != nullptr, EESEN_ERR_INVALID, "null CMVN vectors");
    }
    EESEN_REQUIRE(T > 0, EESEN_ERR_INVALID, "every utterance is empty after the front end");
    const int tb = tap <= nst ? tap : -1;   // the tapped boundary (a plain submit has boundary 0 only)
    EESEN_REQUIRE(tb < 0 || S <= 65535, EESEN_ERR_INVALID, "the statistics tap takes at most 65535 utterances per batch");
    if (h.kind) {   // the waveforms are [samples x 1]: their sample offsets are boundary 0's, written again as they are
      h.fb = fbank_layout(frames, S, fb_plan->dim, [this](int n) { return fb_plan->num_frames(n); }, t.off, t.prefix, t.fb_off);
      for (int s = 0; s < S; ++s) t.ids[s] = fb_next_id + s;
    }
    if (h.kind == kHeadFbankPitch) {
      require_same_rate();
      h.pt = pitch_layout(frames, nullptr, nullptr, fb_next_id, S, pt_plan->opts.delay, pt_plan->proc_dim,
                          [this](int n, int* f1, int* n1, int* n2) { return pt_plan->num_frames(n, f1, n1, n2); }, t.utt);
      for (int s = 0; s < S; ++s) t.proc_off[s] = t.utt[s].proc_off;
    }

    EESEN_HIP_CHECK(hipSetDevice(device));
    if (h.kind) fb_next_id += S;   // every waveform submitted gets a key of its own
    int id = 0;
    Slot& sl = next_slot(&id);
    std::memcpy(sl.tab_h.reserve(tab.size() * 8), tab.data(), tab.size() * 8);
    const float* host = pack(sl, utts, frames, strides, t.off, S, D, total[0]);
    if (Dc) {
      float* cmvn_h = static_cast<float*>(sl.cmvn_h.reserve((size_t)S * 2 * Dc * sizeof(float)));
      for (int s = 0; s < S; ++s) {
        if (frames[s]) std::memcpy(cmvn_h + (size_t)s * 2 * Dc, cmvn[s], (size_t)2 * Dc * sizeof(float));
        else std::memset(cmvn_h + (size_t)s * 2 * Dc, 0, (size_t)2 * Dc * sizeof(float));
      }
      sl.cmvn_d.reserve((size_t)S * 2 * Dc);
      EESEN_HIP_CHECK(hipMemcpyAsync(sl.cmvn_d.p, cmvn_h, (size_t)S * 2 * Dc * sizeof(float), hipMemcpyHostToDevice, copy));
    }
    // even boundaries live in `packed`, odd ones in `packed2`
    size_t cap[2] = {1, nst ? (size_t)1 : 0};
    for (int b = 0; b < nb; ++b) cap[b % 2] = std::max(cap[b % 2], (size_t)total[b]);
    sl.packed.reserve(cap[0]);
    sl.packed2.reserve(cap[1]);
    sl.tab_d.reserve(tab.size());
    const BatchTables d = batch_carve(sl.tab_d.p, nb, S, h.kind);
    if (total[0]) EESEN_HIP_CHECK(hipMemcpyAsync(sl.packed.p, host, (size_t)total[0] * sizeof(float), hipMemcpyHostToDevice, copy));
    EESEN_HIP_CHECK(hipMemcpyAsync(sl.tab_d.p, sl.tab_h.p, tab.size() * 8, hipMemcpyHostToDevice, copy));
    sl.stats_D = 0;
    if (tb == 0) tap_stats(sl, dims, t, d, total.data(), 0, S, sl.packed.p);
    for (int k = 0; k < nst; ++k) {
      if (!total[k + 1]) {   // nothing to write; a tap on it answers zeros
        if (tb == k + 1) tap_stats(sl, dims, t, d, total.data(), k + 1, S, nullptr);
        continue;
      }
      const float* src = k % 2 ? sl.packed2.p : sl.packed.p;
      float* dst = k % 2 ? sl.packed.p : sl.packed2.p;
      long biggest = 0;
      for (int s = 0; s < S; ++s) biggest = std::max(biggest, (long)t.frames[(size_t)(k + 1) * S + s] * dims[k + 1]);
      if (k == 0 && h.kind) {
        head_stage(sl, h, d, S, src, dst, dims[1], biggest);
        if (tb == 1) tap_stats(sl, dims, t, d, total.data(), 1, S, dst);
        continue;
      }
      const StageDev sd{pl[k].kind, pl[k].a, pl[k].b};
      hipLaunchKernelGGL(feat_stage_kernel, stage_grid(biggest, S), dim3(256), 0, copy, sd, scales_d.p ? scales_d.p + pl[k].scale_off : nullptr, src,
                         d.off + (size_t)k * S, d.frames + (size_t)k * S, dims[k], dst, d.off + (size_t)(k + 1) * S,
                         d.frames + (size_t)(k + 1) * S, dims[k + 1], sl.cmvn_d.p);
      check_launch("feat_stage_kernel");
      if (tb == k + 1) tap_stats(sl, dims, t, d, total.data(), k + 1, S, dst);
    }
    assemble(sl, nst % 2 ? sl.packed2.p : sl.packed.p, d.off + (size_t)nst * S, d.frames + (size_t)nst * S, T, S, dims[nst]);
    sl.ready.record(copy);
    sl.in_flight = true;
    return id;
  }
  int submit(const float* const* utts, const int* frames, const int* strides, int S, int D) {
    return stage_batch(std::vector<Stage>(), utts, frames, strides, nullptr, S, D);
  }
  int submit_raw(const float* const* utts, const int* frames, const int* strides, const float* const* cmvn, int S, int D) {
    return stage_batch(pipe, utts, frames, strides, cmvn, S, D);
  }

  Slot& checked(int id) {
    EESEN_REQUIRE(id >= 0 && id < (int)slots.size(), EESEN_ERR_INVALID, "slot id out of range");
    EESEN_REQUIRE(slots[id].in_flight, EESEN_ERR_STATE, "slot holds no submitted batch");
    return slots[id];
  }
  void acquire(int id, float** feats, int* T, int* S, int* ld) {
    Slot& sl = checked(id);
    EESEN_HIP_CHECK(hipSetDevice(device));
    EESEN_HIP_CHECK(hipStreamWaitEvent(compute, sl.ready, 0));  // device-side wait: the host does not block
    *feats = sl.out.p; *T = sl.T; *S = sl.S; *ld = sl.ld;
  }
  void stats(int id, double* out, int* D) {
    EESEN_REQUIRE(tap >= 0, EESEN_ERR_STATE, "the statistics tap is off (eesen_feeder_set_stats_tap)");
    Slot& sl = checked(id);
    EESEN_REQUIRE(sl.stats_D > 0, EESEN_ERR_STATE, "the slot's batch was submitted without the statistics tap");
    sl.ready.wait();
    std::memcpy(out, sl.stats_h.p, (size_t)sl.S * 2 * (sl.stats_D + 1) * sizeof(double));
    *D = sl.stats_D;
  }
  void release(int id) {  // everything enqueued on the compute stream so far may read the slot; later work may not
    Slot& sl = checked(id);
    EESEN_HIP_CHECK(hipSetDevice(device));
    sl.consumed.record(compute);
    sl.has_consumer = true;
  }
};

}  // namespace eesen

struct eesen_feeder : public eesen::Feeder { using eesen::Feeder::Feeder; };

using namespace eesen;

extern "C" {

int eesen_feeder_create(int device, void* compute_stream, int slots, eesen_feeder_t** out) {
  return guard([&] {
    REQ_PTR(out);
    *out = new eesen_feeder(device, compute_stream, slots);
  });
}
int eesen_feeder_destroy(eesen_feeder_t* f) {
  return guard([&] { delete f; });
}
int eesen_feeder_submit(eesen_feeder_t* f, const float* const* utts, const int* frames, const int* strides, int S, int D, int* slot) {
  return guard([&] {
    REQ_PTR(f); REQ_PTR(utts); REQ_PTR(frames); REQ_PTR(slot);
    *slot = f->submit(utts, frames, strides, S, D);
  });
}
int eesen_feeder_set_pipeline(eesen_feeder_t* f, const eesen_feat_stage_t* stages, int n_stages) {
  return guard([&] {
    REQ_PTR(f);
    if (n_stages > 0) REQ_PTR(stages);
    f->set_pipeline(stages, n_stages);
  });
}
int eesen_feeder_set_stats_tap(eesen_feeder_t* f, int boundary) {
  return guard([&] { REQ_PTR(f); f->set_stats_tap(boundary); });
}
int eesen_feeder_stats(eesen_feeder_t* f, int slot, double* stats, int* D) {
  return guard([&] {
    REQ_PTR(f); REQ_PTR(stats); REQ_PTR(D);
    f->stats(slot, stats, D);
  });
}
int eesen_feeder_set_fbank(eesen_feeder_t* f, const eesen_fbank_opts_t* opts) {
  return guard([&] {
    REQ_PTR(f); REQ_PTR(opts);
    f->set_fbank(*opts);
  });
}
int eesen_feeder_set_pitch(eesen_feeder_t* f, const eesen_pitch_opts_t* opts) {
  return guard([&] {
    REQ_PTR(f); REQ_PTR(opts);
    f->set_pitch(*opts);
  });
}
int eesen_feat_paste_frames(const int* frames, int n_inputs, int tolerance, int* out) {
  return guard([&] {
    REQ_PTR(frames); REQ_PTR(out);
    *out = paste_frames(frames, n_inputs, tolerance);
  });
}
// paste-feats on host matrices through feat_paste_kernel: every input packed back to back, one upload, one launch, one copy back
int eesen_paste_feats(int device, void* stream, const float* const* const* inputs, const int* dims, int n_inputs, const int* frames,
                      int S, int tolerance, float* const* out, int* frames_out) {
  return guard([&] {
    REQ_PTR(inputs); REQ_PTR(dims); REQ_PTR(frames);
    EESEN_REQUIRE(n_inputs >= 2 && n_inputs <= kPasteMaxInputs, EESEN_ERR_INVALID, "paste-feats on the device joins 2..4 inputs");
    EESEN_REQUIRE(S > 0 && S <= 65535, EESEN_ERR_INVALID, "1..65535 utterances per call");
    long Dout = 0;
    for (int j = 0; j < n_inputs; ++j) {
      REQ_PTR(inputs[j]);
      EESEN_REQUIRE(dims[j] > 0, EESEN_ERR_INVALID, "an input without columns");
      Dout += dims[j];
    }
    EESEN_REQUIRE(Dout < (1L << 24), EESEN_ERR_INVALID, "too many columns");
    // layout: the inputs' offsets [n x S], the output's offsets [S] and row counts [S]
    std::vector<long> off((size_t)(n_inputs + 1) * S);
    std::vector<int> rows(S);
    std::vector<long> total(n_inputs + 1, 0);
    long biggest = 0;
    for (int s = 0; s < S; ++s) {
      int fr[kPasteMaxInputs];
      for (int j = 0; j < n_inputs; ++j) {
        fr[j] = frames[(size_t)j * S + s];
        EESEN_REQUIRE(fr[j] >= 0, EESEN_ERR_INVALID, "negative frame count");
        EESEN_REQUIRE(fr[j] == 0 || inputs[j][s] != nullptr, EESEN_ERR_INVALID, "null input matrix");
        off[(size_t)j * S + s] = total[j];
      }
      rows[s] = paste_frames(fr, n_inputs, tolerance);
      for (int j = 0; j < n_inputs; ++j) total[j] += (long)rows[s] * dims[j];   // only the rows the join keeps go up
      off[(size_t)n_inputs * S + s] = total[n_inputs];
      total[n_inputs] += (long)rows[s] * Dout;
      biggest = std::max(biggest, (long)rows[s] * Dout);
      EESEN_REQUIRE(rows[s] == 0 || (out && out[s] != nullptr), EESEN_ERR_INVALID, "null output matrix");
      if (frames_out) frames_out[s] = rows[s];
    }
    const long n_out = total[n_inputs];
    if (!n_out) return;            // every utterance dropped: nothing to launch
    require_device(device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    PinBuf host, meta;
    float* h = static_cast<float*>(host.reserve((size_t)n_out * sizeof(float)));   // the inputs side by side take as many floats as the output
    long at = 0;
    std::vector<long> base(n_inputs);
    for (int j = 0; j < n_inputs; ++j) {
      base[j] = at;
      for (int s = 0; s < S; ++s)
        if (rows[s]) std::memcpy(h + at + off[(size_t)j * S + s], inputs[j][s], (size_t)rows[s] * dims[j] * sizeof(float));
      at += total[j];
    }
    const size_t meta_bytes = off.size() * sizeof(long) + (size_t)S * sizeof(int);
    char* m = static_cast<char*>(meta.reserve(meta_bytes));
    std::memcpy(m, off.data(), off.size() * sizeof(long));
    std::memcpy(m + off.size() * sizeof(long), rows.data(), (size_t)S * sizeof(int));
    DevBuf<float> in_d, out_d;
    DevBuf<long> meta_d;
    in_d.reserve((size_t)n_out);
    out_d.reserve((size_t)n_out);
    meta_d.reserve(off.size() + ((size_t)S + 1) / 2);
    EESEN_HIP_CHECK(hipMemcpyAsync(in_d.p, h, (size_t)n_out * sizeof(float), hipMemcpyHostToDevice, st));
    EESEN_HIP_CHECK(hipMemcpyAsync(meta_d.p, m, meta_bytes, hipMemcpyHostToDevice, st));
    PasteArgs pa = PasteArgs();
    pa.n = n_inputs;
    for (int j = 0; j < n_inputs; ++j) { pa.src[j] = in_d.p + base[j]; pa.off[j] = meta_d.p + (size_t)j * S; pa.dim[j] = dims[j]; }
    paste_launch(pa, out_d.p, meta_d.p + (size_t)n_inputs * S, reinterpret_cast<const int*>(meta_d.p + off.size()), (int)Dout, S, biggest, st);
    EESEN_HIP_CHECK(hipMemcpyAsync(h, out_d.p, (size_t)n_out * sizeof(float), hipMemcpyDeviceToHost, st));   // (the staged inputs are consumed by then: one stream)
    EESEN_HIP_CHECK(hipStreamSynchronize(st));
    for (int s = 0; s < S; ++s)
      if (rows[s]) std::memcpy(out[s], h + off[(size_t)n_inputs * S + s], (size_t)rows[s] * Dout * sizeof(float));
  });
}
int eesen_feeder_pipeline_shape(eesen_feeder_t* f, int D_in, int frames_in, int* D_out, int* frames_out) {
  return guard([&] {
    REQ_PTR(f);
    if (D_out) *D_out = f->pipeline_dim(D_in);
    if (frames_out) *frames_out = f->pipeline_frames(frames_in);
  });
}
int eesen_feeder_submit_raw(eesen_feeder_t* f, const float* const* utts, const int* frames, const int* strides,
                            const float* const* cmvn, int S, int D_in, int* slot) {
  return guard([&] {
    REQ_PTR(f); REQ_PTR(utts); REQ_PTR(frames); REQ_PTR(slot);
    *slot = f->submit_raw(utts, frames, strides, cmvn, S, D_in);
  });
}
// the arithmetic of ApplyCmvn, the reference's src/feat/cmvn.cc:78-108: host-only (a few dozen doubles per speaker)
int eesen_cmvn_norm(const double* stats, int rows, int cols, int norm_vars, float* offset_scale) {
  return guard([&] {
    REQ_PTR(stats); REQ_PTR(offset_scale);
    const int dim = cols - 1;
    EESEN_REQUIRE(rows >= 1 && rows <= 2 && dim >= 1, EESEN_ERR_INVALID, "Dim mismatch in ApplyCmvn: cmvn stats must be 1 or 2 rows of dim + 1 columns");
    EESEN_REQUIRE(!(rows == 1 && norm_vars), EESEN_ERR_INVALID, "You requested variance normalization but no variance stats are supplied.");
    const double count = stats[dim];
    EESEN_REQUIRE(count >= 1.0, EESEN_ERR_INVALID, "Insufficient stats for cepstral mean and variance normalization: count = " + std::to_string(count));
    for (int d = 0; d < dim; ++d) {
      double mean = stats[d] / count, offset, scale;
      if (!norm_vars) {
        scale = 1.0;
        offset = -mean;
      } else {
        double var = (stats[(size_t)cols + d] / count) - mean * mean;
        const double floor = 1.0e-20;
        if (var < floor) var = floor;
        scale = 1.0 / std::sqrt(var);
        EESEN_REQUIRE(scale == scale && 1 / scale != 0.0, EESEN_ERR_INVALID, "NaN or infinity in cepstral mean/variance computation");
        offset = -(mean * scale);
      }
      offset_scale[d] = (float)offset;
      offset_scale[dim + d] = (float)scale;
    }
  });
}
int eesen_feeder_acquire(eesen_feeder_t* f, int slot, float** feats_dev, int* T, int* S, int* ld) {
  return guard([&] {
    REQ_PTR(f); REQ_PTR(feats_dev); REQ_PTR(T); REQ_PTR(S); REQ_PTR(ld);
    f->acquire(slot, feats_dev, T, S, ld);
  });
}
int eesen_feeder_release(eesen_feeder_t* f, int slot) {
  return guard([&] { REQ_PTR(f); f->release(slot); });
}

}  // extern "C"
