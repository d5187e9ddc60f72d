// fbank.hip -- log-mel filterbank features of a minibatch of ragged waveforms in one launch (compute-fbank-feats on the device).
//
// Per frame the reference runs ExtractWindow (src/feat/feature-functions.cc:91-167), a split-radix real FFT (srfft.cc), the power
// spectrum, MelBanks::Compute (mel-computations.cc:220-239) and a log (feature-fbank.cc:104-183).  Here one wavefront owns one frame
// and a workgroup of four wavefronts four consecutive frames of the packed minibatch; a frame lives in 1.5 N floats of LDS:
//   x[0 .. N)      the window: raw samples, then (in place, from the last sample down, as the reference's Preemphasize runs) the
//                  DC-free, pre-emphasised, windowed and zero-padded frame, then -- read as N/2 complex numbers
//                  z[n] = x[2n] + i x[2n+1] -- the complex FFT of N/2 points that stands in for the real FFT of N;
//   pw[0 .. N/2)   the power spectrum of bins 0 .. N/2-1 (the reference's filters never reach the Nyquist bin).
// The FFT is radix-2 decimation in frequency, in place: natural order in, bit-reversed order out, so there is no permutation pass --
// the real-split pass that forms X[k] from Z[k] and Z[N/2-k] reads through __brev.  Complex elements are 8 bytes (ds_read_b64,
// bank = (addr/4) mod 64): a pass whose half-size is 32 or more reads 32 consecutive elements per lane group and is conflict-free;
// the five passes below that read two runs that share banks (2-way).  Twiddles and the window function come from tables made on the
// host in fp64 and rounded once; the mel matrix is CSR.  No per-lane arrays: everything a lane keeps is a scalar.
#include <cfloat>
#include <cmath>

#include "dither.h"
#include "fbank.h"

namespace eesen {
namespace {

struct FbankArgs {
  const float* wave; const long* off; const int* nsamp; const int* prefix; const unsigned long long* ids;
  float* out; const long* out_off;
  const float* window; const float* tw; const int* bins; const float* weights;
  int S, total_frames, shift, length, N, log2M, num_bins, dim;
  int snip_edges, remove_dc, use_energy, raw_energy, htk_compat, use_log;
  float dither, preemph, energy_floor, log_energy_floor, log_flt_min;
  unsigned long long seed;
};

__device__ __forceinline__ float wave_sum(float v) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void fbank_kernel(FbankArgs a) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int N = a.N, M = N >> 1, L = a.length;
  float* x = lds + wv * (N + M);
  float* pw = x + N;
  // a wavefront past the last frame recomputes the last one and stores nothing: every wavefront reaches every barrier
  int g = blockIdx.x * kFbankFramesPerBlock + wv;
  const bool live = g < a.total_frames;
  if (!live) g = a.total_frames - 1;
  int lo = 0, hi = a.S - 1;   // the utterance s with prefix[s] <= g < prefix[s + 1]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a.prefix[mid + 1] > g) hi = mid; else lo = mid + 1;
  }
  const int s = lo, f = g - a.prefix[s], n = a.nsamp[s];
  const float* w = a.wave + a.off[s];
  // snip_edges: the window starts at f * shift; otherwise it is centred on shift * (f + 0.5) and reflected at both ends
  const int begin = a.snip_edges ? f * a.shift : f * a.shift + (a.shift >> 1) - L / 2;
  const unsigned long long key = a.dither != 0.f ? mix64(mix64(a.seed) + (a.ids ? a.ids[s] : (unsigned long long)s)) : 0ull;

  float sum = 0.f;
  for (int i = lane; i < N; i += 64) {
    float v = 0.f;
    if (i < L) {
      int j = begin + i;
      if (j < 0) j = (-j) % n;                       // (the % only bites for a waveform shorter than a frame)
      else if (j >= n) j = n - 1 - ((j - n) % n);
      v = w[j];
      if (a.dither != 0.f) v += dither_gauss(key, f, i) * a.dither;
    }
    x[i] = v;
    sum += v;
  }
  const float mean = a.remove_dc ? wave_sum(sum) / L : 0.f;
  __syncthreads();

  // DC removal, raw energy, pre-emphasis and the window function, from the last chunk down: element i needs the DC-free x[i - 1],
  // which a lower chunk still holds unmodified (within a chunk every lane has read before any lane writes)
  float raw_e = 0.f, win_e = 0.f;
  for (int base = ((L - 1) >> 6) << 6; base >= 0; base -= 64) {
    const int i = base + lane;
    float y = 0.f;
    if (i < L) {
      const float c = x[i] - mean, p = x[i ? i - 1 : 0] - mean;
      raw_e += c * c;
      y = (c - a.preemph * p) * a.window[i];
      win_e += y * y;
    }
    __syncthreads();
    if (i < L) x[i] = y;
  }
  __syncthreads();

  // complex FFT of M points over z[n] = x[2n] + i x[2n + 1]
  float2* z = reinterpret_cast<float2*>(x);
  const float2* twM = reinterpret_cast<const float2*>(a.tw);          // exp(-2 pi i k / M), k < M / 2
  const float2* twN = reinterpret_cast<const float2*>(a.tw + M);      // exp(-2 pi i k / N), k < M
  for (int h = M >> 1, stride = 1; h >= 1; h >>= 1, stride <<= 1) {
    for (int j = lane; j < (M >> 1); j += 64) {
      const int p = j & (h - 1), i0 = ((j - p) << 1) + p, i1 = i0 + h;
      const float2 u = z[i0], v = z[i1], t = twM[p * stride];
      const float dx = u.x - v.x, dy = u.y - v.y;
      z[i0] = make_float2(u.x + v.x, u.y + v.y);
      z[i1] = make_float2(dx * t.x - dy * t.y, dx * t.y + dy * t.x);
    }
    __syncthreads();
  }
  // real split: X[k] = E[k] + exp(-2 pi i k / N) O[k], E = (Z[k] + conj Z[M-k]) / 2, O = (Z[k] - conj Z[M-k]) / 2i; |X[k]|^2
  const int sh = 32 - a.log2M;
  for (int k = lane; k < M; k += 64) {
    const float2 A = z[__brev((unsigned)k) >> sh];
    float pk;
    if (k == 0) {
      pk = (A.x + A.y) * (A.x + A.y);
    } else {
      const float2 B = z[__brev((unsigned)(M - k)) >> sh], t = twN[k];
      const float ex = 0.5f * (A.x + B.x), ey = 0.5f * (A.y - B.y);
      const float ox = 0.5f * (A.y + B.y), oy = -0.5f * (A.x - B.x);
      const float xr = ex + (t.x * ox - t.y * oy), xi = ey + (t.x * oy + t.y * ox);
      pk = xr * xr + xi * xi;
    }
    pw[k] = pk;
  }
  __syncthreads();

  float* row = a.out + a.out_off[s] + (long)f * a.dim;
  const int nb = a.num_bins, col0 = (a.use_energy && !a.htk_compat) ? 1 : 0;
  for (int j = lane; j < nb; j += 64) {
    const int fi = a.bins[j], sz = a.bins[nb + j];
    const float* wt = a.weights + a.bins[2 * nb + j];
    float e = 0.f;
    for (int i = 0; i < sz; ++i) e += wt[i] * pw[fi + i];
    if (a.use_log) e = e > FLT_MIN ? logf(e) : a.log_flt_min;      // ApplyFloor(FLT_MIN), ApplyLog
    if (live) row[col0 + j] = e;
  }
  if (a.use_energy) {
    const float e = wave_sum(a.raw_energy ? raw_e : win_e);
    float le = e > FLT_MIN ? logf(e) : a.log_flt_min;
    if (a.energy_floor > 0.f && le < a.log_energy_floor) le = a.log_energy_floor;
    if (live && lane == 0) row[a.htk_compat ? nb : 0] = le;
  }
}

}  // namespace

void FbankDev::upload(const FbankPlan& p) {
  const size_t nb = p.first.size();
  window.reserve(p.window.size());
  twiddle.reserve(p.twiddle.size());
  weights.reserve(p.weights.size());
  bins.reserve(3 * nb);
  std::vector<int> b(p.first);
  b.insert(b.end(), p.size.begin(), p.size.end());
  b.insert(b.end(), p.woff.begin(), p.woff.end());
  EESEN_HIP_CHECK(hipMemcpy(window.p, p.window.data(), p.window.size() * sizeof(float), hipMemcpyHostToDevice));
  EESEN_HIP_CHECK(hipMemcpy(twiddle.p, p.twiddle.data(), p.twiddle.size() * sizeof(float), hipMemcpyHostToDevice));
  EESEN_HIP_CHECK(hipMemcpy(weights.p, p.weights.data(), p.weights.size() * sizeof(float), hipMemcpyHostToDevice));
  EESEN_HIP_CHECK(hipMemcpy(bins.p, b.data(), b.size() * sizeof(int), hipMemcpyHostToDevice));
}

void fbank_launch(const FbankPlan& p, const FbankDev& d, const float* wave, const long* off, const int* nsamp, const int* prefix,
                  const unsigned long long* ids, int S, int total_frames, float* out, const long* out_off, hipStream_t st) {
  if (total_frames <= 0) return;
  const eesen_fbank_opts_t& o = p.opts;
  FbankArgs a;
  a.wave = wave; a.off = off; a.nsamp = nsamp; a.prefix = prefix; a.ids = ids; a.out = out; a.out_off = out_off;
  a.window = d.window.p; a.tw = d.twiddle.p; a.bins = d.bins.p; a.weights = d.weights.p;
  a.S = S; a.total_frames = total_frames; a.shift = p.shift; a.length = p.length; a.N = p.N;
  a.log2M = 0;
  while ((2 << a.log2M) < p.N) ++a.log2M;
  a.num_bins = o.num_bins; a.dim = p.dim;
  a.snip_edges = o.snip_edges != 0; a.remove_dc = o.remove_dc_offset != 0; a.use_energy = o.use_energy != 0;
  a.raw_energy = o.raw_energy != 0; a.htk_compat = o.htk_compat != 0; a.use_log = o.use_log_fbank != 0;
  a.dither = o.dither; a.preemph = o.preemph_coeff; a.energy_floor = o.energy_floor; a.log_energy_floor = p.log_energy_floor;
  a.log_flt_min = logf(FLT_MIN);
  a.seed = o.dither_seed;
  const size_t lds = (size_t)kFbankFramesPerBlock * (p.N + p.N / 2) * sizeof(float);   // 6 KB at N = 256 .. 48 KB at N = 2048
  hipLaunchKernelGGL(fbank_kernel, dim3(cdiv(total_frames, kFbankFramesPerBlock)), dim3(64 * kFbankFramesPerBlock), lds, st, a);
  check_launch("fbank_kernel");
}

}  // namespace eesen
