// cmvn_stats.hip -- per-utterance CMVN statistics of a ragged minibatch on the device: AccCmvnStats of the reference
// (src/feat/cmvn.cc:30-62) for every utterance of a packed batch, and the stand-alone calls of include/eesen_hip.h over it.  The
// feeder's tap (feeder.hip) launches the same kernels on the boundary it holds in HBM.
//
// The reference adds, per row t and column d, the FLOAT products x * w and (x * x) * w to double accumulators, skips rows whose weight
// is zero, and adds w to the count.  Here every product is formed in fp32 exactly so and widened before its first add; no sum is ever
// held in fp32.  No floating-point atomics: a workgroup owns a chunk of an utterance's rows, its threads add their rows in row order,
// the row groups of a workgroup meet in LDS in a fixed tree, and a second launch adds the chunks of an utterance in chunk order.  Where
// the chunks begin is a function of the utterance's frame count and D (cmvn_stats.h), so an utterance's statistics are the same bits
// alone, in any batch and at any position.
//
// The batches are small (5 to 25 MB): the launches and the longest utterance's tail decide the time, not the bandwidth.  The other
// decomposition, one workgroup per utterance reducing in LDS and no second launch, was built and timed beside this one with
// scripts/cmvn_stats_probe.py before it was taken out: 11.6 us against 7.4 at 32 x 1000 x 43, 43.4 against 12.1 at 64 x 3000 x 43 and
// 25.0 against 7.9 at 32 x 1000 x 120 (all but S of the 256 CUs idle, one dependent chain per utterance).  Rows of 43
// or 23 floats are not 16-byte aligned, so loads are plain floats, consecutive lanes on consecutive columns of one row and the next
// row group right behind (215 of 256 lanes busy at D = 43, 240 at D = 40 and 120).
#include <cstring>
#include <vector>

#include "cmvn_stats.h"
#include "guard.h"

namespace eesen {
namespace {

// One workgroup: rows [c * chunk_rows, ...) of utterance blockIdx.y into its partial matrix [2][D + 1].
__global__ __launch_bounds__(kCmvnThreads) void cmvn_acc_kernel(const float* __restrict__ x, const long* __restrict__ off,
                                                                const int* __restrict__ frames, const float* __restrict__ w, int D,
                                                                int chunk_rows, double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double sh[2][kCmvnThreads];
  const int s = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
  const int F = frames[s];
  const int r0 = c * chunk_rows;
  const int r1 = min(F, r0 + chunk_rows);
  if (r0 >= F) return;                                  // (the whole workgroup: no barrier is left waiting)
  const long P = off[s] / D;                            // rows in front of the utterance
  const float* base = x + off[s];
  const float* wt = w ? w + P : nullptr;
  const int ld = D + 1;
  double* o = out + ((size_t)(P / chunk_rows) + s + c) * 2 * ld;

  // the count: the sum of the weights that are not zero (adding a zero changes nothing), or the rows
  if (wt) {
    double cnt = 0.0;
    for (int t = r0 + tid; t < r1; t += kCmvnThreads) cnt += (double)wt[t];
    sh[0][tid] = cnt;
    for (int h = kCmvnThreads / 2; h > 0; h >>= 1) {
      __syncthreads();
      if (tid < h) sh[0][tid] += sh[0][tid + h];
    }
    if (tid == 0) { o[D] = sh[0][0]; o[ld + D] = 0.0; }
    __syncthreads();
  } else if (tid == 0) {
    o[D] = (double)(r1 - r0);
    o[ld + D] = 0.0;
  }

  const int CW = min(D, kCmvnThreads);                  // columns of one tile
  const int rpp = kCmvnThreads / CW;                    // row groups side by side
  const int g = tid / CW;
  for (int c0 = 0; c0 < D; c0 += CW) {
    const int col = c0 + tid % CW;
    const bool active = g < rpp && col < D;
    double s1 = 0.0, s2 = 0.0;
    if (active) {
      const float* p = base + col;
      if (wt) {
#pragma unroll 4
        for (int t = r0 + g; t < r1; t += rpp) {
          const float v = p[(long)t * D], wv = wt[t];
          if (wv != 0.f) {                              // a row of weight 0 is skipped, not multiplied (cmvn.cc:59)
            const float m = v * wv, q = (v * v) * wv;
            s1 += (double)m;
            s2 += (double)q;
          }
        }
      } else {
#pragma unroll 4
        for (int t = r0 + g; t < r1; t += rpp) {
          const float v = p[(long)t * D];
          const float q = v * v;
          s1 += (double)v;
          s2 += (double)q;
        }
      }
    }
    sh[0][tid] = s1;
    sh[1][tid] = s2;
    for (int n = rpp; n > 1;) {                         // the row groups of a column, halved in a fixed order
      const int h = (n + 1) >> 1;
      __syncthreads();
      if (active && g + h < n) {
        sh[0][tid] += sh[0][tid + h * CW];
        sh[1][tid] += sh[1][tid + h * CW];
      }
      n = h;
    }
    if (active && g == 0) {
      o[col] = sh[0][tid];
      o[ld + col] = sh[1][tid];
    }
    __syncthreads();
  }
}

// stats[s] <- the partial matrices of utterance s, added in chunk order; none (no frame): zeros
__global__ __launch_bounds__(kCmvnThreads) void cmvn_finish_kernel(const double* __restrict__ partials, const long* __restrict__ off,
                                                                   const int* __restrict__ frames, int D, int chunk_rows,
                                                                   double* __restrict__ stats) {
  const int s = blockIdx.y;
  const int n = 2 * (D + 1);
  const int j = blockIdx.x * kCmvnThreads + threadIdx.x;
  if (j >= n) return;
  const int nc = (frames[s] + chunk_rows - 1) / chunk_rows;
  const double* p = partials + ((size_t)(off[s] / D / chunk_rows) + s) * n + j;
  double v = 0.0;
#pragma unroll 4
  for (int c = 0; c < nc; ++c) v += p[(size_t)c * n];
  stats[(size_t)s * n + j] = v;
}

}  // namespace

void cmvn_stats_launch(const float* x, const long* off, const int* frames, const float* w, int S, int D, int max_frames, int chunk_rows,
                       double* partials, double* stats, hipStream_t st) {
  EESEN_REQUIRE(S > 0 && S <= 65535 && D > 0, EESEN_ERR_INVALID, "1..65535 utterances per launch, at least one column");
  EESEN_REQUIRE(chunk_rows > 0, EESEN_ERR_INVALID, "at least one row per chunk");
  if (max_frames > 0) {
    hipLaunchKernelGGL(cmvn_acc_kernel, dim3(cmvn_chunks(max_frames, chunk_rows), S), dim3(kCmvnThreads), 0, st, x, off, frames, w, D,
                       chunk_rows, partials);
    check_launch("cmvn_acc_kernel");
  }
  hipLaunchKernelGGL(cmvn_finish_kernel, dim3(cdiv(2 * (D + 1), kCmvnThreads), S), dim3(kCmvnThreads), 0, st, partials, off, frames, D,
                     chunk_rows, stats);
  check_launch("cmvn_finish_kernel");
}

namespace {

// The stand-alone call: the matrices packed back to back (rows made contiguous), one weight per row when any utterance has weights,
// the offsets and frame counts in one block; one upload each, the launches, the statistics back.  bench_iters > 0: eesen_cmvn_stats_bench.
void cmvn_stats_host(int device, void* stream, const float* const* utts, const int* frames, const int* strides, const float* const* weights,
                     int S, int D, double* stats, int bench_iters, float* avg_ms) {
  EESEN_REQUIRE(S > 0 && S <= 65535, EESEN_ERR_INVALID, "1..65535 utterances per call");
  EESEN_REQUIRE(D > 0 && D < (1 << 24), EESEN_ERR_INVALID, "1..2^24 - 1 feature columns");
  std::vector<long> off(S);
  long total = 0, rows = 0;
  int max_frames = 0;
  bool weighted = false;
  for (int s = 0; s < S; ++s) {
    EESEN_REQUIRE(frames[s] >= 0, EESEN_ERR_INVALID, "negative frame count");
    EESEN_REQUIRE(frames[s] == 0 || utts[s] != nullptr, EESEN_ERR_INVALID, "null utterance matrix");
    EESEN_REQUIRE(!strides || frames[s] == 0 || strides[s] >= D, EESEN_ERR_INVALID, "row stride smaller than the feature dimension");
    off[s] = total;
    total += (long)frames[s] * D;
    rows += frames[s];
    max_frames = std::max(max_frames, frames[s]);
    weighted = weighted || (weights && weights[s] && frames[s]);
  }
  EESEN_REQUIRE(rows < (1L << 31), EESEN_ERR_INVALID, "too many frames in one call");
  const size_t nstats = (size_t)S * 2 * (D + 1);
  const int chunk_rows = cmvn_chunk_rows(D);
  require_device(device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  PinBuf host, tab_h, stats_h;
  const size_t nw = weighted ? (size_t)rows : 0;
  float* h = static_cast<float*>(host.reserve(((size_t)total + nw + 1) * sizeof(float)));
  float* wh = h + total;
  for (int s = 0; s < S; ++s) {
    const int st_ = strides ? strides[s] : D;
    if (st_ == D) { if (frames[s]) std::memcpy(h + off[s], utts[s], (size_t)frames[s] * D * sizeof(float)); }
    else for (int t = 0; t < frames[s]; ++t) std::memcpy(h + off[s] + (long)t * D, utts[s] + (long)t * st_, (size_t)D * sizeof(float));
    if (weighted) {
      float* ws = wh + off[s] / D;
      if (weights[s]) { if (frames[s]) std::memcpy(ws, weights[s], (size_t)frames[s] * sizeof(float)); }
      else std::fill(ws, ws + frames[s], 1.0f);         // x * 1 and (x * x) * 1 are x and x * x
    }
  }
  const size_t tab_words = (size_t)S + ((size_t)S + 1) / 2;
  long* th = static_cast<long*>(tab_h.reserve(tab_words * 8));
  std::memcpy(th, off.data(), (size_t)S * 8);
  std::memcpy(th + S, frames, (size_t)S * sizeof(int));
  DevBuf<float> x_d;
  DevBuf<long> tab_d;
  DevBuf<double> part_d, stats_d;
  x_d.reserve((size_t)total + nw + 1);
  tab_d.reserve(tab_words);
  stats_d.reserve(nstats);
  part_d.reserve(cmvn_partial_doubles(rows, S, D, chunk_rows));
  EESEN_HIP_CHECK(hipMemcpyAsync(x_d.p, h, ((size_t)total + nw + 1) * sizeof(float), hipMemcpyHostToDevice, st));
  EESEN_HIP_CHECK(hipMemcpyAsync(tab_d.p, th, tab_words * 8, hipMemcpyHostToDevice, st));
  auto launch = [&] {
    cmvn_stats_launch(x_d.p, tab_d.p, reinterpret_cast<const int*>(tab_d.p + S), weighted ? x_d.p + total : nullptr, S, D, max_frames,
                      chunk_rows, part_d.p, stats_d.p, st);
  };
  launch();
  if (bench_iters > 0) {
    DevEvent t0(true), t1(true);
    t0.record(st);
    for (int i = 0; i < bench_iters; ++i) launch();
    t1.record(st);
    t1.wait();
    float ms = 0.f;
    EESEN_HIP_CHECK(hipEventElapsedTime(&ms, t0, t1));
    *avg_ms = ms / bench_iters;
    return;
  }
  double* sh = static_cast<double*>(stats_h.reserve(nstats * sizeof(double)));
  EESEN_HIP_CHECK(hipMemcpyAsync(sh, stats_d.p, nstats * sizeof(double), hipMemcpyDeviceToHost, st));
  EESEN_HIP_CHECK(hipStreamSynchronize(st));
  std::memcpy(stats, sh, nstats * sizeof(double));
}

}  // namespace
}  // namespace eesen

using namespace eesen;

extern "C" {

int eesen_cmvn_stats_parallel(int device, void* stream, const float* const* utts, const int* frames, const int* strides,
                              const float* const* weights, int S, int D, double* stats) {
  return guard([&] {
    REQ_PTR(utts); REQ_PTR(frames); REQ_PTR(stats);
    cmvn_stats_host(device, stream, utts, frames, strides, weights, S, D, stats, 0, nullptr);
  });
}
int eesen_cmvn_stats_bench(int device, void* stream, const float* const* utts, const int* frames, int S, int D, int iters, float* avg_ms) {
  return guard([&] {
    REQ_PTR(utts); REQ_PTR(frames); REQ_PTR(avg_ms);
    EESEN_REQUIRE(iters > 0, EESEN_ERR_INVALID, "at least one timed launch");
    *avg_ms = 0.f;
    cmvn_stats_host(device, stream, utts, frames, nullptr, nullptr, S, D, nullptr, iters, avg_ms);
  });
}

}  // extern "C"
