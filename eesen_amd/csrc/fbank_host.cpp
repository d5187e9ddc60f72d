// fbank_host.cpp -- host side of the filterbank extractor: options, the reference's checks, the window / twiddle / mel tables, and
// the stand-alone eesen_fbank_* calls of include/eesen_hip.h.  The kernel is in fbank.hip.
#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "fbank.h"
#include "guard.h"

namespace eesen {
namespace {

constexpr double kTwoPi = 6.283185307179586476925286766559005;

inline float mel_scale(float freq) { return 1127.0f * logf(1.0f + freq / 700.0f); }              // mel-computations.h:50-52
inline float inverse_mel_scale(float mel) { return 700.0f * (expf(mel / 1127.0f) - 1.0f); }      // :46-48

// MelBanks::VtlnWarpFreq, mel-computations.cc:144-205
float vtln_warp_freq(float vtln_low_cutoff, float vtln_high_cutoff, float low_freq, float high_freq, float vtln_warp_factor, float freq) {
  if (freq < low_freq || freq > high_freq) return freq;
  EESEN_REQUIRE(vtln_low_cutoff > low_freq, EESEN_ERR_INVALID, "be sure to set the --vtln-low option higher than --low-freq");
  EESEN_REQUIRE(vtln_high_cutoff < high_freq, EESEN_ERR_INVALID, "be sure to set the --vtln-high option lower than --high-freq [or negative]");
  const float one = 1.0f;
  const float l = vtln_low_cutoff * std::max(one, vtln_warp_factor);
  const float h = vtln_high_cutoff * std::min(one, vtln_warp_factor);
  const float scale = 1.0 / vtln_warp_factor;
  const float Fl = scale * l, Fh = scale * h;
  EESEN_REQUIRE(l > low_freq && h < high_freq, EESEN_ERR_INVALID, "VTLN inflection points outside the mel range");
  const float scale_left = (Fl - low_freq) / (l - low_freq);
  const float scale_right = (high_freq - Fh) / (high_freq - h);
  if (freq < l) return low_freq + scale_left * (freq - low_freq);
  if (freq < h) return scale * freq;
  return high_freq + scale_right * (freq - high_freq);
}
float vtln_warp_mel_freq(float vl, float vh, float lo, float hi, float warp, float mel) {
  return mel_scale(vtln_warp_freq(vl, vh, lo, hi, warp, inverse_mel_scale(mel)));
}

int window_size(const eesen_fbank_opts_t& o) { return static_cast<int>(o.samp_freq * 0.001 * o.frame_length_ms); }   // feature-functions.h:122-124
int window_shift(const eesen_fbank_opts_t& o) { return static_cast<int>(o.samp_freq * 0.001 * o.frame_shift_ms); }
int round_up_pow2(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

void check_frame_opts(const eesen_fbank_opts_t& o) {
  EESEN_REQUIRE(o.samp_freq > 0.f && o.frame_shift_ms > 0.f && o.frame_length_ms > 0.f, EESEN_ERR_INVALID, "sample frequency, frame length and frame shift must be positive");
  EESEN_REQUIRE(o.round_to_power_of_two != 0, EESEN_ERR_INVALID, "--round-to-power-of-two=false is not supported");
  EESEN_REQUIRE(o.htk_mode == 0, EESEN_ERR_INVALID, "htk_mode is not supported");
  const int L = window_size(o);
  EESEN_REQUIRE(L > 0 && window_shift(o) > 0, EESEN_ERR_INVALID, "frame length and frame shift must be at least one sample");
  const int N = round_up_pow2(L);
  EESEN_REQUIRE(N >= 256 && N <= 2048, EESEN_ERR_INVALID, "the padded window size must be 256, 512, 1024 or 2048 samples (got " + std::to_string(N) + ")");
  EESEN_REQUIRE(o.window_type >= EESEN_WINDOW_HAMMING && o.window_type <= EESEN_WINDOW_RECTANGULAR, EESEN_ERR_INVALID, "Invalid window type");
  EESEN_REQUIRE(o.preemph_coeff >= 0.f && o.preemph_coeff <= 1.f, EESEN_ERR_INVALID, "pre-emphasis coefficient must be in [0, 1]");
  EESEN_REQUIRE(o.dither >= 0.f, EESEN_ERR_INVALID, "dither must not be negative");
}

}  // namespace

void mel_banks(const eesen_fbank_opts_t& o, std::vector<int>* first, std::vector<int>* size, std::vector<float>* weights) {
  check_frame_opts(o);
  const int num_bins = o.num_bins;
  EESEN_REQUIRE(num_bins >= 3, EESEN_ERR_INVALID, "Must have at least 3 mel bins");
  const float sample_freq = o.samp_freq;
  const int window_length_padded = round_up_pow2(window_size(o));
  const int num_fft_bins = window_length_padded / 2;
  const float nyquist = 0.5 * sample_freq;
  const float low_freq = o.low_freq;
  const float high_freq = o.high_freq > 0.0 ? o.high_freq : nyquist + o.high_freq;
  EESEN_REQUIRE(!(low_freq < 0.0 || low_freq >= nyquist || high_freq <= 0.0 || high_freq > nyquist || high_freq <= low_freq), EESEN_ERR_INVALID,
                "Bad values in options: low-freq " + std::to_string(low_freq) + " and high-freq " + std::to_string(high_freq) + " vs. nyquist " + std::to_string(nyquist));
  const float fft_bin_width = sample_freq / window_length_padded;
  const float mel_low_freq = mel_scale(low_freq), mel_high_freq = mel_scale(high_freq);
  const float mel_freq_delta = (mel_high_freq - mel_low_freq) / (num_bins + 1);
  const float vtln_low = o.vtln_low;
  float vtln_high = o.vtln_high;
  if (vtln_high < 0.0) vtln_high += nyquist;
  const float warp = o.vtln_warp;
  EESEN_REQUIRE(warp > 0.f, EESEN_ERR_INVALID, "the VTLN warp factor must be positive");
  EESEN_REQUIRE(!(warp != 1.0 && (vtln_low < 0.0 || vtln_low <= low_freq || vtln_low >= high_freq || vtln_high <= 0.0 || vtln_high >= high_freq || vtln_high <= vtln_low)),
                EESEN_ERR_INVALID, "Bad values in options: vtln-low " + std::to_string(vtln_low) + " and vtln-high " + std::to_string(vtln_high) + ", versus low-freq " +
                std::to_string(low_freq) + " and high-freq " + std::to_string(high_freq));
  first->assign(num_bins, 0);
  size->assign(num_bins, 0);
  weights->clear();
  std::vector<float> this_bin(num_fft_bins);
  for (int bin = 0; bin < num_bins; ++bin) {
    float left_mel = mel_low_freq + bin * mel_freq_delta, center_mel = mel_low_freq + (bin + 1) * mel_freq_delta,
          right_mel = mel_low_freq + (bin + 2) * mel_freq_delta;
    if (warp != 1.0) {
      left_mel = vtln_warp_mel_freq(vtln_low, vtln_high, low_freq, high_freq, warp, left_mel);
      center_mel = vtln_warp_mel_freq(vtln_low, vtln_high, low_freq, high_freq, warp, center_mel);
      right_mel = vtln_warp_mel_freq(vtln_low, vtln_high, low_freq, high_freq, warp, right_mel);
    }
    int first_index = -1, last_index = -1;
    for (int i = 0; i < num_fft_bins; ++i) {
      const float freq = fft_bin_width * i;
      const float mel = mel_scale(freq);
      this_bin[i] = 0.f;
      if (mel > left_mel && mel < right_mel) {
        this_bin[i] = mel <= center_mel ? (mel - left_mel) / (center_mel - left_mel) : (right_mel - mel) / (right_mel - center_mel);
        if (first_index == -1) first_index = i;
        last_index = i;
      }
    }
    EESEN_REQUIRE(first_index != -1 && last_index >= first_index, EESEN_ERR_INVALID, "You may have set --num-mel-bins too large.");
    (*first)[bin] = first_index;
    (*size)[bin] = last_index + 1 - first_index;
    weights->insert(weights->end(), this_bin.begin() + first_index, this_bin.begin() + last_index + 1);
  }
}

FbankPlan::FbankPlan(const eesen_fbank_opts_t& o) : opts(o) {
  check_frame_opts(o);
  shift = window_shift(o);
  length = window_size(o);
  N = round_up_pow2(length);
  dim = o.num_bins + (o.use_energy ? 1 : 0);
  if (o.energy_floor > 0.0) log_energy_floor = logf(o.energy_floor);
  mel_banks(o, &first, &size, &weights);
  woff.resize(first.size());
  int w = 0;
  for (size_t j = 0; j < first.size(); ++j) { woff[j] = w; w += size[j]; }
  // FeatureWindowFunction, feature-functions.cc:67-85: fp64, rounded once
  window.resize(length);
  for (int i = 0; i < length; ++i) {
    const double c = cos(kTwoPi * static_cast<float>(i) / (length - 1));
    double v = 1.0;
    if (o.window_type == EESEN_WINDOW_HANNING) v = 0.5 - 0.5 * c;
    else if (o.window_type == EESEN_WINDOW_HAMMING) v = 0.54 - 0.46 * c;
    else if (o.window_type == EESEN_WINDOW_POVEY) v = pow(0.5 - 0.5 * c, 0.85);
    window[i] = static_cast<float>(v);
  }
  const int M = N / 2;
  twiddle.resize((size_t)M + 2 * (size_t)M);
  for (int k = 0; k < M / 2; ++k) {
    twiddle[2 * k] = static_cast<float>(cos(-kTwoPi * k / M));
    twiddle[2 * k + 1] = static_cast<float>(sin(-kTwoPi * k / M));
  }
  for (int k = 0; k < M; ++k) {
    twiddle[M + 2 * k] = static_cast<float>(cos(-kTwoPi * k / N));
    twiddle[M + 2 * k + 1] = static_cast<float>(sin(-kTwoPi * k / N));
  }
}

int FbankPlan::num_frames(int nsamp) const {
  if (opts.snip_edges) return nsamp < length ? 0 : 1 + (nsamp - length) / shift;
  return (int)(nsamp * 1.0f / shift + 0.5f);
}

// The stand-alone extractor: one staging area, synchronous per call (the feeder carries its own slots).
struct Fbank {
  FbankPlan plan;
  FbankDev dev;
  int device;
  hipStream_t stream;
  PinBuf wave_h, out_h, tab_h;
  DevBuf<float> wave_d, out_d;
  DevBuf<long> tab_d;           // the batch's tables (feat_layout.h)

  bool on_device = false;       // the tables go up with the first compute(): options, shapes and filters need no device

  Fbank(int dev_, void* st, const eesen_fbank_opts_t& o) : plan(o), device(dev_), stream(static_cast<hipStream_t>(st)) {
    EESEN_REQUIRE(dev_ >= 0, EESEN_ERR_INVALID, "device index out of range");
  }
  ~Fbank() {
    if (!on_device) return;
    (void)hipSetDevice(device);
    (void)hipStreamSynchronize(stream);
  }

  // bench_iters > 0: the microbenchmark of eesen_fbank_bench -- the same staging, one warm-up launch, then bench_iters launches
  // between two events, and no copy back
  void compute(const float* const* waves, const int* nsamp, const unsigned long long* utt_ids, int S, float* const* out_host,
               int bench_iters = 0, float* avg_ms = nullptr) {
    EESEN_REQUIRE(S > 0, EESEN_ERR_INVALID, "need at least one waveform");
    if (!on_device) {
      require_device(device);
      dev.upload(plan);
      on_device = true;
    }
    EESEN_HIP_CHECK(hipSetDevice(device));
    // the batch's tables as the feeder's filterbank head lays them out: one boundary (the samples), one block, one upload
    const size_t words = batch_words(1, S, kHeadFbank);
    const BatchTables h = batch_carve(tab_h.reserve(words * 8), 1, S, kHeadFbank);
    const FbankTotals tot = fbank_layout(nsamp, S, plan.dim, [this](int n) { return plan.num_frames(n); }, h.off, h.prefix, h.fb_off);
    for (int s = 0; s < S; ++s) {
      EESEN_REQUIRE(nsamp[s] == 0 || waves[s] != nullptr, EESEN_ERR_INVALID, "null waveform");
      EESEN_REQUIRE(h.prefix[s + 1] == h.prefix[s] || bench_iters > 0 || (out_host && out_host[s] != nullptr), EESEN_ERR_INVALID, "null output matrix");
      h.frames[s] = nsamp[s];
      h.ids[s] = key_of(utt_ids, 0, s);
    }
    if (!tot.frames) return;
    float* wh = static_cast<float*>(wave_h.reserve((size_t)tot.samp * sizeof(float)));
    for (int s = 0; s < S; ++s)
      if (nsamp[s]) std::memcpy(wh + h.off[s], waves[s], (size_t)nsamp[s] * sizeof(float));
    float* oh = static_cast<float*>(out_h.reserve((size_t)tot.out * sizeof(float)));
    wave_d.reserve((size_t)tot.samp);
    out_d.reserve((size_t)tot.out);
    tab_d.reserve(words);
    const BatchTables d = batch_carve(tab_d.p, 1, S, kHeadFbank);
    EESEN_HIP_CHECK(hipMemcpyAsync(wave_d.p, wh, (size_t)tot.samp * sizeof(float), hipMemcpyHostToDevice, stream));
    EESEN_HIP_CHECK(hipMemcpyAsync(tab_d.p, h.off, words * 8, hipMemcpyHostToDevice, stream));
    auto launch = [&] { fbank_launch(plan, dev, wave_d.p, d.off, d.frames, d.prefix, d.ids, S, tot.frames, out_d.p, d.fb_off, stream); };
    launch();
    if (bench_iters > 0) {
      DevEvent t0(true), t1(true);
      t0.record(stream);
      for (int i = 0; i < bench_iters; ++i) launch();
      t1.record(stream);
      t1.wait();
      float ms = 0.f;
      EESEN_HIP_CHECK(hipEventElapsedTime(&ms, t0, t1));
      *avg_ms = ms / bench_iters;
      return;
    }
    EESEN_HIP_CHECK(hipMemcpyAsync(oh, out_d.p, (size_t)tot.out * sizeof(float), hipMemcpyDeviceToHost, stream));
    EESEN_HIP_CHECK(hipStreamSynchronize(stream));
    for (int s = 0; s < S; ++s) {
      const long n = (long)(h.prefix[s + 1] - h.prefix[s]) * plan.dim;
      if (n) std::memcpy(out_host[s], oh + h.fb_off[s], (size_t)n * sizeof(float));
    }
  }
};

}  // namespace eesen

struct eesen_fbank : public eesen::Fbank { using eesen::Fbank::Fbank; };

using namespace eesen;

extern "C" {

int eesen_fbank_opts_default(eesen_fbank_opts_t* o) {
  return guard([&] {
    REQ_PTR(o);
    std::memset(o, 0, sizeof(*o));
    o->samp_freq = 16000.f; o->frame_shift_ms = 10.f; o->frame_length_ms = 25.f; o->dither = 1.f; o->preemph_coeff = 0.97f;
    o->remove_dc_offset = 1; o->window_type = EESEN_WINDOW_POVEY; o->round_to_power_of_two = 1; o->snip_edges = 1;
    o->num_bins = 23; o->low_freq = 20.f; o->high_freq = 0.f; o->vtln_low = 100.f; o->vtln_high = -500.f; o->htk_mode = 0;
    o->use_energy = 0; o->energy_floor = 0.f; o->raw_energy = 1; o->htk_compat = 0; o->use_log_fbank = 1;
    o->vtln_warp = 1.f; o->dither_seed = 0;
  });
}
int eesen_fbank_create(int device, void* stream, const eesen_fbank_opts_t* opts, eesen_fbank_t** out) {
  return guard([&] {
    REQ_PTR(opts); REQ_PTR(out);
    *out = new eesen_fbank(device, stream, *opts);
  });
}
int eesen_fbank_destroy(eesen_fbank_t* fb) {
  return guard([&] { delete fb; });
}
int eesen_fbank_shape(eesen_fbank_t* fb, int nsamp, int* frames, int* dim) {
  return guard([&] {
    REQ_PTR(fb);
    EESEN_REQUIRE(nsamp >= 0, EESEN_ERR_INVALID, "negative sample count");
    if (frames) *frames = fb->plan.num_frames(nsamp);
    if (dim) *dim = fb->plan.dim;
  });
}
int eesen_fbank_compute(eesen_fbank_t* fb, const float* const* waves, const int* nsamp, const unsigned long long* utt_ids, int S,
                        float* const* out_host) {
  return guard([&] {
    REQ_PTR(fb); REQ_PTR(waves); REQ_PTR(nsamp);
    fb->compute(waves, nsamp, utt_ids, S, out_host);
  });
}
int eesen_fbank_bench(eesen_fbank_t* fb, const float* const* waves, const int* nsamp, int S, int iters, float* avg_ms) {
  return guard([&] {
    REQ_PTR(fb); REQ_PTR(waves); REQ_PTR(nsamp); REQ_PTR(avg_ms);
    EESEN_REQUIRE(iters > 0, EESEN_ERR_INVALID, "at least one timed launch");
    *avg_ms = 0.f;
    fb->compute(waves, nsamp, nullptr, S, nullptr, iters, avg_ms);
  });
}
int eesen_fbank_mel_banks(const eesen_fbank_opts_t* opts, int* first, int* size, float* weights, int weights_cap, int* n_weights) {
  return guard([&] {
    REQ_PTR(opts);
    std::vector<int> f, z;
    std::vector<float> w;
    mel_banks(*opts, &f, &z, &w);
    if (first) std::copy(f.begin(), f.end(), first);
    if (size) std::copy(z.begin(), z.end(), size);
    if (n_weights) *n_weights = (int)w.size();
    if (weights) {
      EESEN_REQUIRE(weights_cap >= (int)w.size(), EESEN_ERR_INVALID, "weight buffer too small");
      std::copy(w.begin(), w.end(), weights);
    }
  });
}

}  // extern "C"
