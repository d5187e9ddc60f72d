// pitch.h -- what the host part of the pitch extractor (pitch_host.cpp) hands to its kernels (pitch.hip).
#pragma once
#include <vector>

#include "common.h"
#include "feat_layout.h"   // PitchUtt, PitchTotals, kPitchMaxStates, kPitchMaxFrames

namespace eesen {

// The validated options in the units the kernels work in, plus the host tables they read (fp64 on the host, rounded to fp32 once).
struct PitchPlan {
  eesen_pitch_opts_t opts;
  int rate_in = 0, rate_out = 0;             // integer sample rates
  int in_unit = 0, out_unit = 0;             // samples of either rate in the repeating unit (rate / gcd): out_unit filter phases
  int window = 0, shift = 0;                 // NccfWindowSize(), NccfWindowShift(), in down-sampled samples
  int first_lag = 0, last_lag = 0, num_lags = 0, full = 0;   // integer lags measured; full = window + last_lag
  int states = 0;                            // size of the lag grid
  int proc_dim = 0;
  float factor = 0.f;                        // penalty_factor * ln(1 + delta_pitch)^2, rounded as the reference rounds it
  std::vector<float> lags;                   // [states] seconds
  std::vector<int> ph_first, ph_size, ph_off;    // down-sampler: per phase, the first input index (relative to the unit), taps, offset
  std::vector<float> ph_w;
  std::vector<int> up_first, up_size, up_off;    // CSR up-sampler: output lag i reads integer-lag columns up_first[i] ..
  std::vector<float> up_w;

  explicit PitchPlan(const eesen_pitch_opts_t& o);
  long num_down(long nsamp, bool flush) const;   // GetNumOutputSamples, resample.cc:56-100
  // frames in all and (f1) of the first pass; n1 / n2: down-sampled samples before and after the flush
  int num_frames(int nsamp, int* f1 = nullptr, int* n1 = nullptr, int* n2 = nullptr) const;
};

std::vector<float> pitch_lags(const eesen_pitch_opts_t& o);   // SelectLags in the reference's float arithmetic

struct PitchSums { double sum1, sq1, sum2, sq2; };   // of the down-sampled signal without and with the flushed tail

struct PitchDev {
  DevBuf<float> ph_w, up_w, lags;
  DevBuf<int> tabs;                          // ph_first | ph_size | ph_off | up_first | up_size | up_off
  void upload(const PitchPlan& p);
};
constexpr int kPitchFramesPerBlock = 4;      // NCCF kernel: one wavefront per frame

struct PitchBufs {
  const PitchUtt* utt; int S; int total_frames;
  const float* wave; float* down; PitchSums* sums;
  float* nccf_pitch; float* nccf_pov; float* avg_norm_prod;    // [total_frames x states] twice, [total_frames]
  unsigned short* backptr;                                     // [total_frames x states]
  float* fwd; int* track; int* taken;                          // [S x states], [total_frames], [S]
  float* raw;                                                  // [total_frames x 2]
  double* scan;                                                // [2 x (total_frames + S)] prefix sums of the post-processing
  float* proc;                                                 // the processed matrices, back to back
};
void pitch_downsample_launch(const PitchPlan& p, const PitchDev& d, const PitchBufs& b, hipStream_t st);
void pitch_nccf_launch(const PitchPlan& p, const PitchDev& d, const PitchBufs& b, hipStream_t st);
void pitch_viterbi_launch(const PitchPlan& p, const PitchDev& d, const PitchBufs& b, hipStream_t st);
void pitch_process_launch(const PitchPlan& p, const PitchBufs& b, hipStream_t st);   // utt[s].frames rows of b.raw from row utt[s].prefix
// down-sample, NCCF, Viterbi and, asked for, the post-processing, in that order on one stream
void pitch_track_launch(const PitchPlan& p, const PitchDev& d, const PitchBufs& b, bool process, hipStream_t st);

// The tracker's device buffers for one batch: the stand-alone extractor holds one set, the feeder one per staging slot.
struct PitchScratch {
  DevBuf<float> down, nccf_pitch, nccf_pov, avg, fwd, raw, proc;
  DevBuf<PitchSums> sums;
  DevBuf<unsigned short> backptr;
  DevBuf<int> track, taken;
  DevBuf<double> scan;
  // sized for the batch and handed to the kernels; diag: the search's forward costs and track as well; search = false: the
  // post-processing alone, which needs no NCCF
  PitchBufs reserve(const PitchPlan& p, const PitchTotals& t, int S, const PitchUtt* utt_d, const float* wave, bool diag = false, bool search = true);
};

}  // namespace eesen
