// fbank.h -- what the host part of the filterbank extractor (fbank_host.cpp) hands to its kernel (fbank.hip).
#pragma once
#include <vector>

#include "common.h"
#include "feat_layout.h"

namespace eesen {

// The validated options in the units the kernel works in, plus the host tables it reads (fp64 on the host, rounded to fp32 once).
struct FbankPlan {
  eesen_fbank_opts_t opts;
  int shift = 0, length = 0, N = 0;        // WindowShift(), WindowSize(), PaddedWindowSize()
  int dim = 0;                             // num_bins + use_energy
  float log_energy_floor = 0.f;
  std::vector<float> window;               // [length]
  std::vector<float> twiddle;              // [N/2] (cos, sin) of -2 pi k / (N/2), k < N/4, then [N] of -2 pi k / N, k < N/2
  std::vector<int> first, size, woff;      // CSR mel matrix: bin j covers fft bins first[j] .. first[j] + size[j] - 1
  std::vector<float> weights;

  explicit FbankPlan(const eesen_fbank_opts_t& o);
  int num_frames(int nsamp) const;         // NumFrames, feature-functions.cc:29-48
};

// MelBanks::MelBanks (mel-computations.cc:32-135) in the reference's float arithmetic
void mel_banks(const eesen_fbank_opts_t& o, std::vector<int>* first, std::vector<int>* size, std::vector<float>* weights);

// Device tables of one extractor and the launch over a packed minibatch (fbank.hip).
struct FbankDev {
  DevBuf<float> window, twiddle, weights;
  DevBuf<int> bins;                        // first | size | woff, num_bins each
  void upload(const FbankPlan& p);
};
constexpr int kFbankFramesPerBlock = 4;    // one wavefront per frame
// wave: the packed samples; off[s] / nsamp[s]: where utterance s starts and how long it is; prefix[s]: frames in front of
// utterance s (prefix[S] = total_frames); ids: the dither keys (NULL: s); out_off[s]: where its [frames x dim] matrix starts.
void fbank_launch(const FbankPlan& p, const FbankDev& d, const float* wave, const long* off, const int* nsamp, const int* prefix,
                  const unsigned long long* ids, int S, int total_frames, float* out, const long* out_off, hipStream_t st);

}  // namespace eesen
