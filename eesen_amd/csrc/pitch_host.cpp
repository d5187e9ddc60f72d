// pitch_host.cpp -- host side of the pitch extractor: options, the refusals, the down-sampler's phase tables, the lag grid, the
// up-sampler's CSR table, frame counts, and the stand-alone eesen_pitch_* calls of include/eesen_hip.h.  The kernels are in pitch.hip.
#include <cmath>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "guard.h"
#include "pitch.h"

namespace eesen {
namespace {

constexpr double kTwoPi = 6.283185307179586476925286766559005;
constexpr double kPi = 3.141592653589793238462643383279503;

// the Hann-windowed sinc of LinearResample::FilterFunc / ArbitraryResample::FilterFunc (resample.cc:244-257, :351-364), in fp64
double filter_func(double t, double cutoff, int zeros) {
  const double window = std::fabs(t) < zeros / (2.0 * cutoff) ? 0.5 * (1.0 + cos(kTwoPi * cutoff / zeros * t)) : 0.0;
  const double filter = t != 0.0 ? sin(kTwoPi * cutoff * t) / (kPi * t) : 2.0 * cutoff;
  return filter * window;
}

void check_opts(const eesen_pitch_opts_t& o) {
  EESEN_REQUIRE(o.preemph_coeff == 0.f, EESEN_ERR_INVALID, "--preemphasis-coefficient is deprecated in the reference and not supported: it must be 0");
  EESEN_REQUIRE(o.frames_per_chunk == 0, EESEN_ERR_INVALID, "--frames-per-chunk emulates online operation, which is not supported: it must be 0");
  EESEN_REQUIRE(o.simulate_first_pass_online == 0, EESEN_ERR_INVALID, "--simulate-first-pass-online emulates online operation, which is not supported");
  EESEN_REQUIRE(o.nccf_ballast_online == 0, EESEN_ERR_INVALID, "--nccf-ballast-online emulates online operation, which is not supported");
  EESEN_REQUIRE(o.samp_freq >= 1.f && o.resample_freq >= 1.f && o.samp_freq == std::floor(o.samp_freq) && o.resample_freq == std::floor(o.resample_freq) &&
                o.samp_freq < 1.0e6f && o.resample_freq < 1.0e6f, EESEN_ERR_INVALID, "sample frequency and resample frequency must be whole numbers of hertz");
  EESEN_REQUIRE(o.frame_shift_ms > 0.f && o.frame_length_ms > 0.f, EESEN_ERR_INVALID, "frame length and frame shift must be positive");
  EESEN_REQUIRE(o.lowpass_cutoff > 0.f && o.resample_freq > 2.f * o.lowpass_cutoff, EESEN_ERR_INVALID, "--resample-frequency must be more than twice --lowpass-cutoff");
  EESEN_REQUIRE(o.samp_freq > 2.f * o.lowpass_cutoff, EESEN_ERR_INVALID, "--sample-frequency must be more than twice --lowpass-cutoff");
  EESEN_REQUIRE(o.lowpass_filter_width > 0 && o.upsample_filter_width > 0, EESEN_ERR_INVALID, "filter widths must be positive");
  EESEN_REQUIRE(o.min_f0 > 0.f && o.max_f0 > o.min_f0, EESEN_ERR_INVALID, "need 0 < --min-f0 < --max-f0");
  EESEN_REQUIRE(o.soft_min_f0 >= 0.f && o.soft_min_f0 <= o.min_f0, EESEN_ERR_INVALID, "--soft-min-f0 must not exceed --min-f0");
  EESEN_REQUIRE(o.delta_pitch > 0.f && o.penalty_factor >= 0.f && o.nccf_ballast >= 0.f, EESEN_ERR_INVALID, "--delta-pitch must be positive, --penalty-factor and --nccf-ballast not negative");
  EESEN_REQUIRE(o.recompute_frame >= 0, EESEN_ERR_INVALID, "--recompute-frame must not be negative");
  const int dim = (o.add_pov_feature != 0) + (o.add_normalized_log_pitch != 0) + (o.add_delta_pitch != 0) + (o.add_raw_log_pitch != 0);
  EESEN_REQUIRE(dim > 0, EESEN_ERR_INVALID, "At least one of the pitch features should be chosen. Check your post-process-pitch options.");
  EESEN_REQUIRE(o.delta_window > 0 && o.delta_window < 1000, EESEN_ERR_INVALID, "--delta-window must be in 1 .. 999");
  EESEN_REQUIRE(o.normalization_left_context >= 0 && o.normalization_right_context >= 0 && o.delay >= 0 && o.delay < 100000, EESEN_ERR_INVALID,
                "normalization contexts and --delay must not be negative");
  EESEN_REQUIRE(o.delta_pitch_noise_stddev >= 0.f, EESEN_ERR_INVALID, "--delta-pitch-noise-stddev must not be negative");
}

}  // namespace

std::vector<float> pitch_lags(const eesen_pitch_opts_t& o) {
  check_opts(o);
  const float min_lag = 1.0 / o.max_f0, max_lag = 1.0 / o.min_f0;
  std::vector<float> lags;
  for (float lag = min_lag; lag <= max_lag; lag *= 1.0 + o.delta_pitch) {
    lags.push_back(lag);
    EESEN_REQUIRE(lags.size() <= (size_t)kPitchMaxStates, EESEN_ERR_INVALID,
                  "more than " + std::to_string(kPitchMaxStates) + " lag states: one workgroup of the search holds no more (raise --delta-pitch or narrow --min-f0 .. --max-f0)");
  }
  EESEN_REQUIRE(!lags.empty(), EESEN_ERR_INVALID, "no lag states");
  return lags;
}

PitchPlan::PitchPlan(const eesen_pitch_opts_t& o) : opts(o) {
  lags = pitch_lags(o);
  states = (int)lags.size();
  rate_in = (int)o.samp_freq;
  rate_out = (int)o.resample_freq;
  const int g = std::gcd(rate_in, rate_out);
  in_unit = rate_in / g;
  out_unit = rate_out / g;
  window = static_cast<int>(o.resample_freq * 0.001 * o.frame_length_ms);     // pitch-functions.h:199-205
  shift = static_cast<int>(o.resample_freq * 0.001 * o.frame_shift_ms);
  EESEN_REQUIRE(window > 0 && shift > 0, EESEN_ERR_INVALID, "frame length and frame shift must be at least one down-sampled sample");
  const double half = o.upsample_filter_width / (2.0 * o.resample_freq);
  first_lag = (int)ceil(o.resample_freq * (1.0 / o.max_f0 - half));           // :715-720
  last_lag = (int)floor(o.resample_freq * (1.0 / o.min_f0 + half));
  EESEN_REQUIRE(first_lag >= 0 && last_lag >= first_lag, EESEN_ERR_INVALID, "the lag range is empty or starts below zero (lower --max-f0 or --upsample-filter-width)");
  num_lags = last_lag + 1 - first_lag;
  full = window + last_lag;
  EESEN_REQUIRE((size_t)kPitchFramesPerBlock * (full + 2 * num_lags) * sizeof(float) <= 64 * 1024, EESEN_ERR_INVALID,
                "window plus longest lag is too long for the NCCF kernel's LDS (lower --frame-length or --resample-frequency, or raise --min-f0)");
  proc_dim = (o.add_pov_feature != 0) + (o.add_normalized_log_pitch != 0) + (o.add_delta_pitch != 0) + (o.add_raw_log_pitch != 0);
  const float delta_pitch_sq = (float)(log(1.0 + o.delta_pitch) * log(1.0 + o.delta_pitch));    // :316-317
  factor = delta_pitch_sq * o.penalty_factor;

  // LinearResample::SetIndexesAndWeights (resample.cc:102-131): one weight vector per output phase, fp64, rounded once
  const double lp_width = o.lowpass_filter_width / (2.0 * o.lowpass_cutoff);
  for (int i = 0; i < out_unit; ++i) {
    const double t = i / (double)rate_out;
    const int lo = (int)ceil((t - lp_width) * rate_in), hi = (int)floor((t + lp_width) * rate_in);
    ph_first.push_back(lo);
    ph_size.push_back(hi - lo + 1);
    ph_off.push_back((int)ph_w.size());
    for (int j = lo; j <= hi; ++j) ph_w.push_back((float)(filter_func(j / (double)rate_in - t, o.lowpass_cutoff, o.lowpass_filter_width) / rate_in));
  }
  // ArbitraryResample (resample.cc:260-344) on the lags, offset so that integer lag first_lag is column 0: CSR
  const double rf = o.resample_freq, up_cutoff = 0.5 * rf, up_width = o.upsample_filter_width / (2.0 * up_cutoff);
  const float offset = -first_lag / o.resample_freq;
  for (int i = 0; i < states; ++i) {
    const double t = (float)(lags[i] + offset);
    const int lo = std::max((int)ceil(rf * (t - up_width)), 0), hi = std::min((int)floor(rf * (t + up_width)), num_lags - 1);
    EESEN_REQUIRE(hi >= lo, EESEN_ERR_INVALID, "a lag state has no integer lag within the up-sampling filter");
    up_first.push_back(lo);
    up_size.push_back(hi - lo + 1);
    up_off.push_back((int)up_w.size());
    for (int j = lo; j <= hi; ++j) up_w.push_back((float)(filter_func(t - j / rf, up_cutoff, o.upsample_filter_width) / rf));
  }
}

long PitchPlan::num_down(long nsamp, bool flush) const {
  const long tick = (long)rate_in / std::gcd(rate_in, rate_out) * rate_out;       // lcm
  long length = nsamp * (tick / rate_in);
  if (!flush) {
    const float window_width = opts.lowpass_filter_width / (2.0 * opts.lowpass_cutoff);
    length -= (long)floorf(window_width * (float)tick);
  }
  if (length <= 0) return 0;
  const long per_out = tick / rate_out;
  long last = length / per_out;
  if (last * per_out == length) --last;
  return last + 1;
}

int PitchPlan::num_frames(int nsamp, int* f1_out, int* n1_out, int* n2_out) const {
  const long n1 = num_down(nsamp, false), n2 = num_down(nsamp, true);
  EESEN_REQUIRE(n2 < (1L << 30), EESEN_ERR_INVALID, "waveform too long");
  // NumFramesAvailable (pitch-functions.cc:760-775): the first pass wants window + last_lag samples per frame and always snips;
  // after InputFinished the window alone counts and the frames past the end are zero-padded
  const int f1 = n1 < full ? 0 : (int)((n1 - full) / shift) + 1;
  int fa = 0;
  if (n2 >= window) fa = opts.snip_edges ? (int)((n2 - window) / shift) + 1 : (int)(n2 * 1.0f / shift + 0.5f);
  if (f1_out) *f1_out = f1;
  if (n1_out) *n1_out = (int)n1;
  if (n2_out) *n2_out = (int)n2;
  return std::max(fa, f1);
}

PitchBufs PitchScratch::reserve(const PitchPlan& p, const PitchTotals& t, int S, const PitchUtt* utt_d, const float* wave, bool diag, bool search) {
  const size_t F = (size_t)std::max(t.frames, 1L), ns = search ? (size_t)p.states : 0;
  down.reserve((size_t)std::max(t.down, 1L));
  sums.reserve((size_t)S);
  nccf_pitch.reserve(F * ns);
  nccf_pov.reserve(F * ns);
  avg.reserve(F);
  backptr.reserve(F * ns);
  raw.reserve(F * 2);
  scan.reserve(2 * (F + S));
  proc.reserve((size_t)std::max(t.proc, 1L));
  taken.reserve((size_t)S);
  if (diag) { fwd.reserve((size_t)S * ns); track.reserve(F); }
  PitchBufs b;
  b.utt = utt_d; b.S = S; b.total_frames = (int)t.frames;
  b.wave = wave; b.down = down.p; b.sums = sums.p;
  b.nccf_pitch = nccf_pitch.p; b.nccf_pov = nccf_pov.p; b.avg_norm_prod = avg.p;
  b.backptr = backptr.p; b.fwd = diag ? fwd.p : nullptr; b.track = diag ? track.p : nullptr; b.taken = taken.p;
  b.raw = raw.p; b.scan = scan.p; b.proc = proc.p;
  return b;
}

void pitch_track_launch(const PitchPlan& p, const PitchDev& d, const PitchBufs& b, bool process, hipStream_t st) {
  pitch_downsample_launch(p, d, b, st);
  pitch_nccf_launch(p, d, b, st);
  pitch_viterbi_launch(p, d, b, st);
  if (process) pitch_process_launch(p, b, st);
}

// The stand-alone extractor: one staging area, synchronous per call.
struct Pitch {
  PitchPlan plan;
  PitchDev dev;
  int device;
  hipStream_t stream;
  bool on_device = false;      // the tables go up with the first compute call: options, shapes and lags need no device
  PinBuf wave_h, out_h, diag_h;
  std::vector<PitchUtt> utts;
  PitchTotals tot;
  DevBuf<PitchUtt> utt_d;
  DevBuf<float> wave_d;
  PitchScratch sc;

  Pitch(int dev_, void* st, const eesen_pitch_opts_t& o) : plan(o), device(dev_), stream(static_cast<hipStream_t>(st)) {
    EESEN_REQUIRE(dev_ >= 0, EESEN_ERR_INVALID, "device index out of range");
  }
  ~Pitch() {
    if (!on_device) return;
    (void)hipSetDevice(device);
    (void)hipStreamSynchronize(stream);
  }

  void to_device() {
    if (!on_device) {
      require_device(device);
      dev.upload(plan);
      on_device = true;
    }
    EESEN_HIP_CHECK(hipSetDevice(device));
  }

  // lays the utterances out; frames[s] given (post-processing alone) or counted from nsamp[s]
  void layout(const int* nsamp, const int* frames, const unsigned long long* ids, int S) {
    EESEN_REQUIRE(S > 0, EESEN_ERR_INVALID, "need at least one utterance");
    utts.assign(S, PitchUtt());
    tot = pitch_layout(nsamp, frames, ids, 0, S, plan.opts.delay, plan.proc_dim,
                       [this](int n, int* f1, int* n1, int* n2) { return plan.num_frames(n, f1, n1, n2); }, utts.data());
    utt_d.reserve((size_t)S);
    EESEN_HIP_CHECK(hipMemcpyAsync(utt_d.p, utts.data(), (size_t)S * sizeof(PitchUtt), hipMemcpyHostToDevice, stream));
    EESEN_HIP_CHECK(hipStreamSynchronize(stream));      // utts is pageable and reused
  }

  // a batch of waveforms laid out, on its way to the device, and the scratch sized for it
  PitchBufs stage(const float* const* waves, const int* nsamp, const unsigned long long* ids, int S, bool diag = false) {
    to_device();
    layout(nsamp, nullptr, ids, S);
    float* wh = static_cast<float*>(wave_h.reserve((size_t)std::max(tot.samp, 1L) * sizeof(float)));
    for (int s = 0; s < S; ++s) {
      EESEN_REQUIRE(utts[s].nsamp == 0 || waves[s] != nullptr, EESEN_ERR_INVALID, "null waveform");
      if (utts[s].nsamp) std::memcpy(wh + utts[s].wave_off, waves[s], (size_t)utts[s].nsamp * sizeof(float));
    }
    wave_d.reserve((size_t)std::max(tot.samp, 1L));
    if (tot.samp) EESEN_HIP_CHECK(hipMemcpyAsync(wave_d.p, wh, (size_t)tot.samp * sizeof(float), hipMemcpyHostToDevice, stream));
    return sc.reserve(plan, tot, S, utt_d.p, wave_d.p, diag);
  }

  // rows and floats per row of utterance s in the matrices handed back
  void copy_out(bool process, float* const* out, const long* out_cap, int* frames_out) {
    const int S = (int)utts.size();
    const int dim = process ? plan.proc_dim : 2;
    const long total = process ? tot.proc : tot.frames * 2;
    for (int s = 0; s < S; ++s) {
      const int rows = utts[s].frames ? utts[s].frames + (process ? plan.opts.delay : 0) : 0;
      EESEN_REQUIRE(rows == 0 || (out && out[s] != nullptr), EESEN_ERR_INVALID, "null output matrix");
      EESEN_REQUIRE(rows == 0 || !out_cap || out_cap[s] >= (long)rows * dim, EESEN_ERR_INVALID, "output matrix too small");
      if (frames_out) frames_out[s] = rows;
    }
    if (!total) return;
    float* oh = static_cast<float*>(out_h.reserve((size_t)total * sizeof(float)));
    EESEN_HIP_CHECK(hipMemcpyAsync(oh, process ? sc.proc.p : sc.raw.p, (size_t)total * sizeof(float), hipMemcpyDeviceToHost, stream));
    EESEN_HIP_CHECK(hipStreamSynchronize(stream));
    for (int s = 0; s < S; ++s) {
      if (!utts[s].frames) continue;
      const long off = process ? utts[s].proc_off : (long)utts[s].prefix * 2;
      const long n = (long)(utts[s].frames + (process ? plan.opts.delay : 0)) * dim;
      std::memcpy(out[s], oh + off, (size_t)n * sizeof(float));
    }
  }

  void compute(const float* const* waves, const int* nsamp, const unsigned long long* ids, int S, bool process, float* const* out,
               const long* out_cap, int* frames_out) {
    pitch_track_launch(plan, dev, stage(waves, nsamp, ids, S), process, stream);
    copy_out(process, out, out_cap, frames_out);
    EESEN_HIP_CHECK(hipStreamSynchronize(stream));
  }

  void process(const float* const* raw, const int* frames, const unsigned long long* ids, int S, float* const* out, const long* out_cap,
               int* frames_out) {
    to_device();
    layout(nullptr, frames, ids, S);
    const PitchBufs b = sc.reserve(plan, tot, S, utt_d.p, nullptr, false, false);
    float* rh = static_cast<float*>(wave_h.reserve((size_t)std::max(tot.frames, 1L) * 2 * sizeof(float)));
    for (int s = 0; s < S; ++s) {
      EESEN_REQUIRE(utts[s].frames == 0 || raw[s] != nullptr, EESEN_ERR_INVALID, "null input matrix");
      for (long k = 0; k < (long)utts[s].frames; ++k)
        EESEN_REQUIRE(raw[s][2 * k + 1] > 0.f, EESEN_ERR_INVALID, "pitch values must be positive");
      if (utts[s].frames) std::memcpy(rh + (long)utts[s].prefix * 2, raw[s], (size_t)utts[s].frames * 2 * sizeof(float));
    }
    if (tot.frames) EESEN_HIP_CHECK(hipMemcpyAsync(sc.raw.p, rh, (size_t)tot.frames * 2 * sizeof(float), hipMemcpyHostToDevice, stream));
    pitch_process_launch(plan, b, stream);
    copy_out(true, out, out_cap, frames_out);
    EESEN_HIP_CHECK(hipStreamSynchronize(stream));
  }

  template <class T>
  void fetch(T* host, const T* devp, size_t n) {
    if (!host || !n) return;
    T* h = static_cast<T*>(diag_h.reserve(n * sizeof(T)));
    EESEN_HIP_CHECK(hipMemcpyAsync(h, devp, n * sizeof(T), hipMemcpyDeviceToHost, stream));
    EESEN_HIP_CHECK(hipStreamSynchronize(stream));
    std::memcpy(host, h, n * sizeof(T));
  }

  void stages(const float* wave, int nsamp, int* counts, float* down, float* nccf_pitch, float* nccf_pov, float* lags, float* avg,
              double* mean_square, float* fwd, unsigned short* backptr, int* track, float* raw, int* taken) {
    EESEN_REQUIRE(nsamp >= 0, EESEN_ERR_INVALID, "negative sample count");
    int f1 = 0, n1 = 0, n2 = 0;
    const int frames = plan.num_frames(nsamp, &f1, &n1, &n2);
    if (counts) { counts[0] = frames; counts[1] = f1; counts[2] = plan.states; counts[3] = n2; counts[4] = n1; }
    if (lags) std::copy(plan.lags.begin(), plan.lags.end(), lags);
    if (!down && !nccf_pitch && !nccf_pov && !avg && !mean_square && !fwd && !backptr && !track && !raw && !taken) return;
    pitch_track_launch(plan, dev, stage(&wave, &nsamp, nullptr, 1, true), false, stream);
    EESEN_HIP_CHECK(hipStreamSynchronize(stream));
    const size_t F = (size_t)frames, ns = (size_t)plan.states;
    fetch(down, sc.down.p, (size_t)n2);
    PitchSums sm;
    fetch(&sm, sc.sums.p, 1);
    if (mean_square) {
      mean_square[0] = n1 ? sm.sq1 / n1 - (sm.sum1 / n1) * (sm.sum1 / n1) : 0.0;
      mean_square[1] = n2 ? sm.sq2 / n2 - (sm.sum2 / n2) * (sm.sum2 / n2) : 0.0;
    }
    fetch(nccf_pitch, sc.nccf_pitch.p, F * ns);
    fetch(nccf_pov, sc.nccf_pov.p, F * ns);
    fetch(avg, sc.avg.p, F);
    fetch(backptr, sc.backptr.p, F * ns);
    fetch(track, sc.track.p, F);
    fetch(raw, sc.raw.p, F * 2);
    if (F) fetch(fwd, sc.fwd.p, ns);
    if (taken) {
      *taken = 0;
      if (F) fetch(taken, sc.taken.p, 1);
    }
  }

  // avg_ms[5]: everything, then each launch alone; one warm-up pass first (it also fills what the later launches read)
  void bench(const float* const* waves, const int* nsamp, int S, int iters, float* avg_ms) {
    const PitchBufs b = stage(waves, nsamp, nullptr, S);
    auto run = [&](int which) {
      if (which == 0 || which == 1) pitch_downsample_launch(plan, dev, b, stream);
      if (which == 0 || which == 2) pitch_nccf_launch(plan, dev, b, stream);
      if (which == 0 || which == 3) pitch_viterbi_launch(plan, dev, b, stream);
      if (which == 0 || which == 4) pitch_process_launch(plan, b, stream);
    };
    run(0);
    for (int which = 0; which < 5; ++which) {
      DevEvent t0(true), t1(true);
      t0.record(stream);
      for (int i = 0; i < iters; ++i) run(which);
      t1.record(stream);
      t1.wait();
      float ms = 0.f;
      EESEN_HIP_CHECK(hipEventElapsedTime(&ms, t0, t1));
      avg_ms[which] = ms / iters;
    }
  }
};

}  // namespace eesen

struct eesen_pitch : public eesen::Pitch { using eesen::Pitch::Pitch; };

using namespace eesen;

extern "C" {

int eesen_pitch_opts_default(eesen_pitch_opts_t* o) {
  return guard([&] {
    REQ_PTR(o);
    std::memset(o, 0, sizeof(*o));
    o->samp_freq = 16000.f; o->frame_shift_ms = 10.f; o->frame_length_ms = 25.f; o->preemph_coeff = 0.f;
    o->min_f0 = 50.f; o->max_f0 = 400.f; o->soft_min_f0 = 10.f; o->penalty_factor = 0.1f;
    o->lowpass_cutoff = 1000.f; o->resample_freq = 4000.f; o->delta_pitch = 0.005f; o->nccf_ballast = 7000.f;
    o->lowpass_filter_width = 1; o->upsample_filter_width = 5;
    o->max_frames_latency = 0; o->frames_per_chunk = 0; o->simulate_first_pass_online = 0;
    o->recompute_frame = 500; o->nccf_ballast_online = 0; o->snip_edges = 1;
    o->pitch_scale = 2.f; o->pov_scale = 2.f; o->pov_offset = 0.f; o->delta_pitch_scale = 10.f; o->delta_pitch_noise_stddev = 0.005f;
    o->normalization_left_context = 75; o->normalization_right_context = 75; o->delta_window = 2; o->delay = 0;
    o->add_pov_feature = 1; o->add_normalized_log_pitch = 1; o->add_delta_pitch = 1; o->add_raw_log_pitch = 0;
    o->noise_seed = 0;
  });
}
int eesen_pitch_create(int device, void* stream, const eesen_pitch_opts_t* opts, eesen_pitch_t** out) {
  return guard([&] {
    REQ_PTR(opts); REQ_PTR(out);
    *out = new eesen_pitch(device, stream, *opts);
  });
}
int eesen_pitch_destroy(eesen_pitch_t* p) {
  return guard([&] { delete p; });
}
int eesen_pitch_shape(eesen_pitch_t* p, int nsamp, int* frames, int* raw_dim, int* processed_dim) {
  return guard([&] {
    REQ_PTR(p);
    EESEN_REQUIRE(nsamp >= 0, EESEN_ERR_INVALID, "negative sample count");
    if (frames) *frames = p->plan.num_frames(nsamp);
    if (raw_dim) *raw_dim = 2;
    if (processed_dim) *processed_dim = p->plan.proc_dim;
  });
}
int eesen_pitch_compute(eesen_pitch_t* p, const float* const* waves, const int* nsamp, const unsigned long long* utt_ids, int S,
                        int process, float* const* out, const long* out_cap, int* frames_out) {
  return guard([&] {
    REQ_PTR(p); REQ_PTR(waves); REQ_PTR(nsamp);
    p->compute(waves, nsamp, utt_ids, S, process != 0, out, out_cap, frames_out);
  });
}
int eesen_pitch_process(eesen_pitch_t* p, const float* const* raw, const int* frames, const unsigned long long* utt_ids, int S,
                        float* const* out, const long* out_cap, int* frames_out) {
  return guard([&] {
    REQ_PTR(p); REQ_PTR(raw); REQ_PTR(frames);
    p->process(raw, frames, utt_ids, S, out, out_cap, frames_out);
  });
}
int eesen_pitch_nccf(eesen_pitch_t* p, const float* wave, int nsamp, int* counts, float* down, float* nccf_pitch, float* nccf_pov,
                     float* lags, float* avg_norm_prod, double* mean_square, float* fwd, unsigned short* backptr, int* track,
                     float* raw, int* taken) {
  return guard([&] {
    REQ_PTR(p);
    EESEN_REQUIRE(nsamp == 0 || wave != nullptr, EESEN_ERR_INVALID, "null waveform");
    p->stages(wave, nsamp, counts, down, nccf_pitch, nccf_pov, lags, avg_norm_prod, mean_square, fwd, backptr, track, raw, taken);
  });
}
int eesen_pitch_lags(const eesen_pitch_opts_t* opts, float* lags, int cap, int* n) {
  return guard([&] {
    REQ_PTR(opts);
    const std::vector<float> l = pitch_lags(*opts);
    if (n) *n = (int)l.size();
    if (lags) {
      EESEN_REQUIRE(cap >= (int)l.size(), EESEN_ERR_INVALID, "lag buffer too small");
      std::copy(l.begin(), l.end(), lags);
    }
  });
}
int eesen_pitch_bench(eesen_pitch_t* p, const float* const* waves, const int* nsamp, int S, int iters, float* avg_ms) {
  return guard([&] {
    REQ_PTR(p); REQ_PTR(waves); REQ_PTR(nsamp); REQ_PTR(avg_ms);
    EESEN_REQUIRE(iters > 0, EESEN_ERR_INVALID, "at least one timed launch");
    for (int i = 0; i < 5; ++i) avg_ms[i] = 0.f;
    p->bench(waves, nsamp, S, iters, avg_ms);
  });
}

}  // extern "C"
