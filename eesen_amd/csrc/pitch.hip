// pitch.hip -- the Kaldi pitch tracker on a minibatch of ragged waveforms (compute-kaldi-pitch-feats | process-kaldi-pitch-feats on
// the device): the offline path of ComputeKaldiPitch (src/feat/pitch-functions.cc:1244-1280) and ProcessPitch (:1536-1549).
//
// Four kernels, one launch of each per minibatch:
//   pitch_downsample_kernel  one workgroup per utterance: LinearResample (resample.cc:31-258) as one weight vector per output phase,
//                            taps added lowest input index first; then the fp64 sums of x and x^2, without and with the flushed
//                            tail, reduced in a fixed tree (so a waveform gives the same bits in any launch).
//   pitch_nccf_kernel        one wavefront per frame, four frames per workgroup (fbank's layout).  The zero-padded window of
//                            window + last_lag samples sits in LDS; the integer lags run across the lanes, and per lag the inner
//                            product and e2 are each a dot product of their own over the window, lowest sample first (x[k] is an
//                            LDS broadcast, x[lag + k] consecutive banks).  Both NCCF rows stay in LDS and are up-sampled to the lag
//                            grid through the CSR table of ArbitraryResample, lag states across the lanes.
//   pitch_viterbi_kernel     the hot path: one workgroup per utterance, one thread per lag state.  See below.
//   pitch_process_kernel     one workgroup per utterance: fp64 prefix sums of pov and pov * log pitch by an LDS scan of 256 frames at
//                            a time, then every output row from differences of them; deltas and noise in the same pass.
//
// The search.  State i of frame t takes the exact minimum over ALL states j of frame t - 1 (the reference's pitch_use_naive_search
// branch; its default branch narrows bounds to the same minimum when there are no ties).  Arithmetic is float32, every operation
// rounded on its own (__fmul_rn / __fadd_rn / __fsub_rn; build.py compiles this file with -ffp-contract=off, which also reaches
// the bodies of those intrinsics in the HIP headers -- a pragma here would not, and they would fuse), in this order:
//     n      = nccf[t][i]                      and, on the frames of a taken energy re-estimate, n = n * scale[t]
//              scale[t] = sqrt((old_ballast + avg_norm_prod[t]) / (new_ballast + avg_norm_prod[t])), correctly rounded / and sqrt
//     local  = (1 - n) + (soft_min_f0 * lag[i]) * n
//     cand_j = ((j - i) * (j - i)) * factor + prev[j]          j = 0, 1, ... ascending; a later j wins only if strictly smaller
//     fwd[i] = cand_best + local
//     prev   = fwd - min_i fwd                                 (min: wavefront reduction, then one LDS exchange)
// prev starts at zero.  (j - i)^2 is exact in float32 (below 2^24).  The previous frame's costs sit in LDS and are read four at a
// time as a broadcast; entries past the last state hold +inf and never win.  Back pointers go out as uint16 [frames x states]; after
// the last frame one thread takes the first minimum of prev and walks them back, writing (NCCF without ballast at the chosen
// state, 1 / lag) per frame.  tests/pitch_restatement.py `search` restates exactly this and reproduces it bit for bit.
// No pruning: the exact bound (a state with cost 0 limits |j - i|) was not built.
#include <cfloat>
#include <cmath>

#include "dither.h"
#include "pitch.h"

namespace eesen {
namespace {

struct PitchArgs {
  PitchBufs b;
  const float* ph_w; const float* up_w; const float* lags; const int* tabs;
  int in_unit, out_unit, window, shift, first_lag, num_lags, full, states, recompute_frame;
  float nccf_ballast, soft_min_f0, factor;
  // post-processing
  int dim, left, right, delta_window, delay, add_pov, add_norm, add_delta, add_raw;
  float pitch_scale, pov_scale, pov_offset, delta_scale, noise_stddev;
  unsigned long long seed;
};

__device__ __forceinline__ float wave_sum(float v) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double mean_square(double sum, double sq, int n) {
  if (n <= 0) return 0.0;
  const double m = sum / n;
  return sq / n - m * m;
}

__global__ __launch_bounds__(256) void pitch_downsample_kernel(PitchArgs a) {
  __shared__ double red[4][256];
  const PitchUtt u = a.b.utt[blockIdx.x];
  const float* w = a.b.wave + u.wave_off;
  float* out = a.b.down + u.down_off;
  const int* ph_first = a.tabs;
  const int* ph_size = a.tabs + a.out_unit;
  const int* ph_off = a.tabs + 2 * a.out_unit;
  double s1 = 0.0, q1 = 0.0, s2 = 0.0, q2 = 0.0;
  for (int k = threadIdx.x; k < u.n2; k += 256) {
    const int unit = k / a.out_unit, ph = k - unit * a.out_unit;
    const long base = (long)ph_first[ph] + (long)unit * a.in_unit;
    const float* wt = a.ph_w + ph_off[ph];
    const int nt = ph_size[ph];
    float acc = 0.f;
    for (int j = 0; j < nt; ++j) {
      const long idx = base + j;
      if (idx >= 0 && idx < u.nsamp) acc += wt[j] * w[idx];    // past either end: zero
    }
    out[k] = acc;
    const double v = acc, vv = v * v;
    if (k < u.n1) { s1 += v; q1 += vv; }
    s2 += v;
    q2 += vv;
  }
  red[0][threadIdx.x] = s1; red[1][threadIdx.x] = q1; red[2][threadIdx.x] = s2; red[3][threadIdx.x] = q2;
  __syncthreads();
  for (int h = 128; h; h >>= 1) {
    if ((int)threadIdx.x < h)
      for (int c = 0; c < 4; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    PitchSums s;
    s.sum1 = red[0][0]; s.sq1 = red[1][0]; s.sum2 = red[2][0]; s.sq2 = red[3][0];
    a.b.sums[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(64 * kPitchFramesPerBlock) void pitch_nccf_kernel(PitchArgs a) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int W = a.window, NL = a.num_lags, full = a.full, ns = a.states;
  float* x = lds + wv * (full + 2 * NL);
  float* ni = x + full;                       // [NL] with the ballast, [NL] without
  // a wavefront past the last frame recomputes the last one and stores nothing: every wavefront reaches every barrier
  int g = blockIdx.x * kPitchFramesPerBlock + wv;
  const bool live = g < a.b.total_frames;
  if (!live) g = a.b.total_frames - 1;
  int lo = 0, hi = a.b.S - 1;                 // the first utterance whose frames end past g
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a.b.utt[mid].prefix + a.b.utt[mid].frames > g) hi = mid; else lo = mid + 1;
  }
  const PitchUtt u = a.b.utt[lo];
  const int f = g - u.prefix;
  const long start = (long)f * a.shift;
  const float* d = a.b.down + u.down_off;

  float sum = 0.f;
  for (int i = lane; i < full; i += 64) {
    const long idx = start + i;
    const float v = idx < u.n2 ? d[idx] : 0.f;   // zero padding past the end (only on the frames the flush adds)
    x[i] = v;
    if (i < W) sum += v;
  }
  const float mean = wave_sum(sum) / (float)W;
  float e1 = 0.f;
  for (int i = lane; i < full; i += 64) {        // the mean of the first W samples comes off all of the window, padding included
    const float v = x[i] - mean;
    x[i] = v;
    if (i < W) e1 += v * v;
  }
  e1 = wave_sum(e1);
  __syncthreads();

  const PitchSums sm = a.b.sums[lo];
  const double ms = f < u.f1 ? mean_square(sm.sum1, sm.sq1, u.n1) : mean_square(sm.sum2, sm.sq2, u.n2);
  const float ballast = (float)((ms * W) * (ms * W) * (double)a.nccf_ballast);
  float norm_sum = 0.f;
  for (int base = 0; base < NL; base += 64) {
    const int l = base + lane;
    if (l < NL) {
      const float* y = x + a.first_lag + l;      // y[k], k < W, ends at first_lag + NL - 1 + W - 1 = full - 1
      float ip = 0.f, e2 = 0.f;
      for (int k = 0; k < W; ++k) {
        const float p = x[k], q = y[k];
        ip += p * q;
        e2 += q * q;
      }
      const float np = e1 * e2;
      const float den = sqrtf(np + ballast), den0 = sqrtf(np);
      ni[l] = den != 0.f ? ip / den : 0.f;
      ni[NL + l] = den0 != 0.f ? ip / den0 : 0.f;
      norm_sum += np;
    }
  }
  norm_sum = wave_sum(norm_sum);
  __syncthreads();

  const int* up_first = a.tabs + 3 * a.out_unit;
  const int* up_size = up_first + ns;
  const int* up_off = up_first + 2 * ns;
  for (int i = lane; i < ns; i += 64) {
    const int fi = up_first[i], sz = up_size[i];
    const float* wt = a.up_w + up_off[i];
    float p = 0.f, q = 0.f;
    for (int j = 0; j < sz; ++j) {
      p += wt[j] * ni[fi + j];
      q += wt[j] * ni[NL + fi + j];
    }
    if (live) {
      a.b.nccf_pitch[(long)g * ns + i] = p;
      a.b.nccf_pov[(long)g * ns + i] = q;
    }
  }
  if (live && lane == 0) a.b.avg_norm_prod[g] = norm_sum / (float)NL;
}

__global__ __launch_bounds__(kPitchMaxStates) void pitch_viterbi_kernel(PitchArgs a) {
  extern __shared__ float lds[];
  const PitchUtt u = a.b.utt[blockIdx.x];
  if (u.frames == 0) return;                    // the whole workgroup
  const int i = threadIdx.x, NSP = blockDim.x, ns = a.states, nw = NSP >> 6;
  const int lane = i & 63, wv = i >> 6;
  float* prev[2] = {lds, lds + NSP};
  float* wmin = lds + 2 * NSP;                  // [2][16]
  const bool valid = i < ns;
  prev[0][i] = valid ? 0.f : INFINITY;
  prev[1][i] = INFINITY;

  // the energy re-estimate of RecomputeBacktraces (pitch-functions.cc:908-1000), decided here per utterance: the frames of the
  // first pass used the mean square without the flushed tail; when that differs from the final one by more than 1 %, their
  // NCCF is rescaled as if the ballast had been the final one
  const PitchSums sm = a.b.sums[blockIdx.x];
  const int n_re = u.f1 < a.recompute_frame ? min(u.frames, a.recompute_frame) : 0;
  int n_scaled = 0;
  float old_b = 0.f, new_b = 0.f;
  if (n_re > 0 && u.f1 > 0) {
    const float m1 = (float)mean_square(sm.sum1, sm.sq1, u.n1), m2 = (float)mean_square(sm.sum2, sm.sq2, u.n2);
    const bool same = m1 == m2 || fabsf(__fsub_rn(m1, m2)) <= __fmul_rn(0.01f, __fadd_rn(fabsf(m1), fabsf(m2)));
    if (!same) {
      const double W = a.window;
      old_b = (float)(((double)m1 * W) * ((double)m1 * W) * (double)a.nccf_ballast);
      new_b = (float)(((double)m2 * W) * ((double)m2 * W) * (double)a.nccf_ballast);
      n_scaled = min(u.f1, n_re);
    }
  }
  if (i == 0 && a.b.taken) a.b.taken[blockIdx.x] = n_scaled > 0;

  const float klag = valid ? __fmul_rn(a.soft_min_f0, a.lags[i]) : 0.f;
  const float fi = (float)i, factor = a.factor;
  const int ns4 = (ns + 3) & ~3;                // <= NSP: NSP is a multiple of 64
  __syncthreads();

  for (int f = 0; f < u.frames; ++f) {
    const long g = (long)u.prefix + f;
    const float* cur = prev[f & 1];
    float* nxt = prev[(f & 1) ^ 1];
    float n = valid ? a.b.nccf_pitch[g * ns + i] : 0.f;
    if (f < n_scaled) {
      const float anp = a.b.avg_norm_prod[g];
      n = __fmul_rn(n, sqrtf(__fadd_rn(old_b, anp) / __fadd_rn(new_b, anp)));
    }
    const float local = __fadd_rn(__fsub_rn(1.f, n), __fmul_rn(klag, n));
    float best = INFINITY;
    int bj = 0;
    for (int j = 0; j < ns4; j += 4) {
      const float4 p = *reinterpret_cast<const float4*>(cur + j);
      const float d0 = (float)j - fi, d1 = d0 + 1.f, d2 = d0 + 2.f, d3 = d0 + 3.f;   // exact: small integers
      const float c0 = __fadd_rn(__fmul_rn(__fmul_rn(d0, d0), factor), p.x);
      const float c1 = __fadd_rn(__fmul_rn(__fmul_rn(d1, d1), factor), p.y);
      const float c2 = __fadd_rn(__fmul_rn(__fmul_rn(d2, d2), factor), p.z);
      const float c3 = __fadd_rn(__fmul_rn(__fmul_rn(d3, d3), factor), p.w);
      if (c0 < best) { best = c0; bj = j; }
      if (c1 < best) { best = c1; bj = j + 1; }
      if (c2 < best) { best = c2; bj = j + 2; }
      if (c3 < best) { best = c3; bj = j + 3; }
    }
    const float fwd = valid ? __fadd_rn(best, local) : INFINITY;
    if (valid) a.b.backptr[g * ns + i] = (unsigned short)bj;
    float m = fwd;
    for (int o = 32; o; o >>= 1) m = fminf(m, __shfl_xor(m, o, 64));
    if (lane == 0) wmin[(f & 1) * 16 + wv] = m;
    __syncthreads();
    m = wmin[(f & 1) * 16];
    for (int w = 1; w < nw; ++w) m = fminf(m, wmin[(f & 1) * 16 + w]);
    nxt[i] = valid ? __fsub_rn(fwd, m) : INFINITY;
    __syncthreads();
  }

  const float* last = prev[u.frames & 1];
  if (valid && a.b.fwd) a.b.fwd[(long)blockIdx.x * ns + i] = last[i];
  if (i == 0) {                                 // (the barrier above ordered every back pointer of this workgroup before these reads)
    int s = 0;
    float best = last[0];
    for (int j = 1; j < ns; ++j)
      if (last[j] < best) { best = last[j]; s = j; }
    for (int f = u.frames - 1; f >= 0; --f) {
      const long g = (long)u.prefix + f;
      if (a.b.track) a.b.track[g] = s;
      a.b.raw[2 * g] = a.b.nccf_pov[g * ns + s];
      a.b.raw[2 * g + 1] = (float)(1.0 / (double)a.lags[s]);
      s = a.b.backptr[g * ns + s];
    }
  }
}

// NccfToPov (pitch-functions.cc:76-86)
__device__ __forceinline__ float nccf_to_pov(float n) {
  double nd = fabs((double)n);
  if (nd > 1.0) nd = 1.0;
  const double r = -5.2 + 5.4 * exp(7.5 * (nd - 1.0)) + 4.8 * nd - 2.0 * exp(-10.0 * nd) + 4.2 * exp(20.0 * (nd - 1.0));
  return (float)(1.0 / (1.0 + exp(-r)));
}
__device__ __forceinline__ float log_pitch(const float* raw, long row) { return (float)log((double)raw[2 * row + 1]); }

__global__ __launch_bounds__(256) void pitch_process_kernel(PitchArgs a) {
  __shared__ double sa[256], sb[256];
  const PitchUtt u = a.b.utt[blockIdx.x];
  const int T = u.frames, tid = threadIdx.x;
  if (T == 0) return;                           // the whole workgroup
  const float* raw = a.b.raw;
  const long row0 = u.prefix;
  // prefix sums P[t] = sum over frames < t, T + 1 entries per utterance
  double* P_pov = a.b.scan + row0 + blockIdx.x;
  double* P_lp = P_pov + (a.b.total_frames + a.b.S);
  if (a.add_norm) {
    double carry_a = 0.0, carry_b = 0.0;
    if (tid == 0) { P_pov[0] = 0.0; P_lp[0] = 0.0; }
    for (int base = 0; base < T; base += 256) {
      const int t = base + tid;
      double va = 0.0, vb = 0.0;
      if (t < T) {
        const float pov = nccf_to_pov(raw[2 * (row0 + t)]);
        va = pov;
        vb = __fmul_rn(pov, log_pitch(raw, row0 + t));
      }
      sa[tid] = va; sb[tid] = vb;
      __syncthreads();
      for (int o = 1; o < 256; o <<= 1) {       // inclusive scan
        double xa = 0.0, xb = 0.0;
        if (tid >= o) { xa = sa[tid - o]; xb = sb[tid - o]; }
        __syncthreads();
        sa[tid] += xa; sb[tid] += xb;
        __syncthreads();
      }
      if (t < T) { P_pov[t + 1] = carry_a + sa[tid]; P_lp[t + 1] = carry_b + sb[tid]; }
      carry_a += sa[255]; carry_b += sb[255];
      __syncthreads();
    }
  }
  __syncthreads();                              // the prefix sums of this workgroup are visible to all of it

  const unsigned long long key = a.noise_stddev != 0.f ? mix64(mix64(a.seed) + u.id) : 0ull;
  const int w = a.delta_window;
  float normalizer = 0.f;
  for (int j = -w; j <= w; ++j) normalizer += (float)(j * j);
  const float inv_norm = (float)(1.0 / normalizer);
  float* out = a.b.proc + u.proc_off;
  for (int r = tid; r < T + a.delay; r += 256) {
    const int t = r < a.delay ? 0 : r - a.delay;
    float* o = out + (long)r * a.dim;
    const float nccf = raw[2 * (row0 + t)], lp = log_pitch(raw, row0 + t);
    int c = 0;
    if (a.add_pov) {                            // NccfToPovFeature (:42-51)
      const float nc = fminf(fmaxf(nccf, -1.f), 1.f);
      const float fv = (float)(pow(1.0001 - (double)nc, 0.15) - 1.0);
      o[c++] = a.pov_scale * fv + a.pov_offset;
    }
    if (a.add_norm) {
      const int b = max(t - a.left, 0), e = min(t + a.right + 1, T);
      const float avg = (float)((P_lp[e] - P_lp[b]) / (P_pov[e] - P_pov[b]));
      o[c++] = (lp - avg) * a.pitch_scale;
    }
    if (a.add_delta) {                          // ComputeDeltas of order 1 on the window clipped to the utterance
      float dl = 0.f;
      for (int j = -w; j <= w; ++j) {
        if (j == 0) continue;
        const int tt = min(max(t + j, 0), T - 1);
        dl += ((float)j * inv_norm) * log_pitch(raw, row0 + tt);
      }
      if (a.noise_stddev != 0.f) dl += dither_gauss(key, t, 0) * a.noise_stddev;
      o[c++] = dl * a.delta_scale;
    }
    if (a.add_raw) o[c++] = lp;
  }
}

PitchArgs make_args(const PitchPlan& p, const PitchDev* d, const PitchBufs& b) {
  const eesen_pitch_opts_t& o = p.opts;
  PitchArgs a;
  a.b = b;
  a.ph_w = d ? d->ph_w.p : nullptr; a.up_w = d ? d->up_w.p : nullptr; a.lags = d ? d->lags.p : nullptr; a.tabs = d ? d->tabs.p : nullptr;
  a.in_unit = p.in_unit; a.out_unit = p.out_unit; a.window = p.window; a.shift = p.shift; a.first_lag = p.first_lag;
  a.num_lags = p.num_lags; a.full = p.full; a.states = p.states; a.recompute_frame = o.recompute_frame;
  a.nccf_ballast = o.nccf_ballast; a.soft_min_f0 = o.soft_min_f0; a.factor = p.factor;
  a.dim = p.proc_dim; a.left = o.normalization_left_context; a.right = o.normalization_right_context;
  a.delta_window = o.delta_window; a.delay = o.delay;
  a.add_pov = o.add_pov_feature != 0; a.add_norm = o.add_normalized_log_pitch != 0; a.add_delta = o.add_delta_pitch != 0;
  a.add_raw = o.add_raw_log_pitch != 0;
  a.pitch_scale = o.pitch_scale; a.pov_scale = o.pov_scale; a.pov_offset = o.pov_offset; a.delta_scale = o.delta_pitch_scale;
  a.noise_stddev = o.delta_pitch_noise_stddev; a.seed = o.noise_seed;
  return a;
}

}  // namespace

void PitchDev::upload(const PitchPlan& p) {
  std::vector<int> t(p.ph_first);
  t.insert(t.end(), p.ph_size.begin(), p.ph_size.end());
  t.insert(t.end(), p.ph_off.begin(), p.ph_off.end());
  t.insert(t.end(), p.up_first.begin(), p.up_first.end());
  t.insert(t.end(), p.up_size.begin(), p.up_size.end());
  t.insert(t.end(), p.up_off.begin(), p.up_off.end());
  ph_w.reserve(p.ph_w.size());
  up_w.reserve(p.up_w.size());
  lags.reserve(p.lags.size());
  tabs.reserve(t.size());
  EESEN_HIP_CHECK(hipMemcpy(ph_w.p, p.ph_w.data(), p.ph_w.size() * sizeof(float), hipMemcpyHostToDevice));
  EESEN_HIP_CHECK(hipMemcpy(up_w.p, p.up_w.data(), p.up_w.size() * sizeof(float), hipMemcpyHostToDevice));
  EESEN_HIP_CHECK(hipMemcpy(lags.p, p.lags.data(), p.lags.size() * sizeof(float), hipMemcpyHostToDevice));
  EESEN_HIP_CHECK(hipMemcpy(tabs.p, t.data(), t.size() * sizeof(int), hipMemcpyHostToDevice));
}

void pitch_downsample_launch(const PitchPlan& p, const PitchDev& d, const PitchBufs& b, hipStream_t st) {
  if (b.S <= 0) return;
  hipLaunchKernelGGL(pitch_downsample_kernel, dim3(b.S), dim3(256), 0, st, make_args(p, &d, b));
  check_launch("pitch_downsample_kernel");
}

void pitch_nccf_launch(const PitchPlan& p, const PitchDev& d, const PitchBufs& b, hipStream_t st) {
  if (b.total_frames <= 0) return;
  const size_t lds = (size_t)kPitchFramesPerBlock * (p.full + 2 * p.num_lags) * sizeof(float);   // 5.3 KB at the defaults
  hipLaunchKernelGGL(pitch_nccf_kernel, dim3(cdiv(b.total_frames, kPitchFramesPerBlock)), dim3(64 * kPitchFramesPerBlock), lds, st,
                     make_args(p, &d, b));
  check_launch("pitch_nccf_kernel");
}

void pitch_viterbi_launch(const PitchPlan& p, const PitchDev& d, const PitchBufs& b, hipStream_t st) {
  if (b.total_frames <= 0) return;
  const int threads = cdiv(p.states, 64) * 64;                                                   // 448 at the default 417 states
  const size_t lds = ((size_t)2 * threads + 32) * sizeof(float);
  hipLaunchKernelGGL(pitch_viterbi_kernel, dim3(b.S), dim3(threads), lds, st, make_args(p, &d, b));
  check_launch("pitch_viterbi_kernel");
}

void pitch_process_launch(const PitchPlan& p, const PitchBufs& b, hipStream_t st) {
  if (b.total_frames <= 0) return;
  hipLaunchKernelGGL(pitch_process_kernel, dim3(b.S), dim3(256), 0, st, make_args(p, nullptr, b));
  check_launch("pitch_process_kernel");
}

}  // namespace eesen
