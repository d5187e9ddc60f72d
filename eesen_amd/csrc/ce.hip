// ce.hip -- frame-level cross-entropy over a padded utterance batch, for gfx950.
//
// Reference arithmetic: CE::EvalParallel, the reference's src/net/ce-loss.cc:94-169.  The reference builds a dense one-hot
// [rows x K] target matrix on the host, copies it to the device and then makes five passes over [rows x K] matrices: copy +
// AddMat (diff = y - onehot), MulRowsVec (padding mask), FindRowMaxId (frame accuracy), and copy + ApplyLog + MulElements +
// MulRowsVec + Sum (objective).  Here ONE kernel reads the posteriors once, fed by rows x 4 bytes of int32 targets and the
// S sequence lengths (row t*S + s is valid iff t < len[s], the reference's frame_mask_host, train-ce-parallel.cc:176-184):
//   * diff = (y - onehot(target)) * mask: the same float operations as AddMat(-1, onehot) then MulRowsVec, so bit for bit;
//     padded rows are written 0 without reading y;
//   * the row's argmax with the FindRowMaxId rule of row_argmax_kernel (ctc.hip): strict `<` in increasing index per lane,
//     the smaller index between lanes on equal values, -1e21 start (cuda-matrix.cc:1045) -- the first maximum;
//   * -log y[target] (fp32 log, as ApplyLog) and the correct flag, summed per wave in row order in fp64 / int64.
// One wavefront per row, four rows per workgroup, a grid-stride loop over a grid that depends on `rows` alone; workgroup
// partials are reduced by a one-workgroup kernel in a fixed order: no atomics, the same inputs give the same bits every run.
// Rows are 16-byte aligned with a pad4 stride everywhere in the library, so the row body moves as float4 (global_load_dwordx4
// / global_store_dwordx4) and only the last K % 4 columns go one float at a time.
#include "kernels.h"

namespace eesen {
namespace {

constexpr int kCeWaves = 4;        // rows in flight per workgroup (one wavefront each)
constexpr int kCeMaxBlocks = 2048; // 8192 wavefronts: 32 per CU on the 256 CUs

__device__ __forceinline__ void take(float v, int k, float& best, int& bi) {
  if (best < v) { best = v; bi = k; }
}

template <bool VEC>
__global__ __launch_bounds__(256) void ce_eval_kernel(const float* __restrict__ y, int ld, int rows, int K, int S,
                                                      const int* __restrict__ lens, const int* __restrict__ tgt,
                                                      float* __restrict__ diff, int ldd, CeSums* __restrict__ part) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int stride = gridDim.x * kCeWaves;
  double obj = 0.0;
  long long correct = 0;
  for (int r = blockIdx.x * kCeWaves + w; r < rows; r += stride) {
    const int t = r / S, s = r - t * S;
    float* dr = diff + (size_t)r * ldd;
    if (t >= lens[s]) {  // padding: MulRowsVec by 0 (ce-loss.cc:123-125), and no statistic
      if (VEC) {
        const int K4 = K >> 2;
        for (int q = lane; q < K4; q += 64) reinterpret_cast<float4*>(dr)[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int k = 4 * K4 + lane; k < K; k += 64) dr[k] = 0.f;
      } else {
        for (int k = lane; k < K; k += 64) dr[k] = 0.f;
      }
      continue;
    }
    const float* yr = y + (size_t)r * ld;
    const int c = tgt[r];
    float best = -1e21f;  // cuda-matrix.cc:1045
    int bi = -1;
    if (VEC) {
      const int K4 = K >> 2;
#pragma unroll 4
      for (int q = lane; q < K4; q += 64) {
        const float4 v = reinterpret_cast<const float4*>(yr)[q];
        const int k = 4 * q;
        take(v.x, k, best, bi); take(v.y, k + 1, best, bi); take(v.z, k + 2, best, bi); take(v.w, k + 3, best, bi);
        float4 d = v;
        const unsigned j = (unsigned)(c - k);
        if (j < 4u) {   // diff = y + (-1) * onehot (AddMat), then * 1 (MulRowsVec)
          if (j == 0) d.x = v.x - 1.f; else if (j == 1) d.y = v.y - 1.f; else if (j == 2) d.z = v.z - 1.f; else d.w = v.w - 1.f;
        }
        reinterpret_cast<float4*>(dr)[q] = d;
      }
      for (int k = 4 * K4 + lane; k < K; k += 64) {
        const float v = yr[k];
        take(v, k, best, bi);
        dr[k] = k == c ? v - 1.f : v;
      }
    } else {
      for (int k = lane; k < K; k += 64) {
        const float v = yr[k];
        take(v, k, best, bi);
        dr[k] = k == c ? v - 1.f : v;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {  // row_argmax_kernel's combine: the smaller index wins a tie
      const float ov = __shfl_xor(best, o);
      const int oi = __shfl_xor(bi, o);
      if (ov > best || (ov == best && oi >= 0 && (bi < 0 || oi < bi))) { best = ov; bi = oi; }
    }
    if (lane == 0) {
      obj += (double)(-logf(yr[c]));   // ApplyLog in fp32 (ce-loss.cc:137-142), summed in fp64
      correct += bi == c;
    }
  }
  __shared__ double s_obj[kCeWaves];
  __shared__ long long s_cor[kCeWaves];
  if (lane == 0) { s_obj[w] = obj; s_cor[w] = correct; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double o = 0.0;
    long long n = 0;
    for (int i = 0; i < kCeWaves; ++i) { o += s_obj[i]; n += s_cor[i]; }
    part[blockIdx.x] = CeSums{o, n};
  }
}

// sums of the workgroup partials in a fixed order: thread i folds i, i + 256, ... then a fixed-shape tree
__global__ __launch_bounds__(256) void ce_reduce_kernel(const CeSums* __restrict__ part, int n, CeSums* __restrict__ out) {
  __shared__ double s_obj[256];
  __shared__ long long s_cor[256];
  double o = 0.0;
  long long c = 0;
  for (int i = threadIdx.x; i < n; i += 256) { o += part[i].obj; c += part[i].correct; }
  s_obj[threadIdx.x] = o;
  s_cor[threadIdx.x] = c;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) { s_obj[threadIdx.x] += s_obj[threadIdx.x + h]; s_cor[threadIdx.x] += s_cor[threadIdx.x + h]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = CeSums{s_obj[0], s_cor[0]};
}

}  // namespace

int ce_eval_blocks(int rows) { return std::max(1, std::min(cdiv(rows, kCeWaves), kCeMaxBlocks)); }

void ce_eval(hipStream_t st, const float* y, int ld, int rows, int K, int S, const int* lens, const int* tgt, float* diff,
             int ldd, CeSums* part, CeSums* out) {
  const int nb = ce_eval_blocks(rows);
  const bool vec = ld % 4 == 0 && ldd % 4 == 0 && reinterpret_cast<uintptr_t>(y) % 16 == 0 && reinterpret_cast<uintptr_t>(diff) % 16 == 0;
  if (vec)
    hipLaunchKernelGGL(ce_eval_kernel<true>, dim3(nb), dim3(256), 0, st, y, ld, rows, K, S, lens, tgt, diff, ldd, part);
  else
    hipLaunchKernelGGL(ce_eval_kernel<false>, dim3(nb), dim3(256), 0, st, y, ld, rows, K, S, lens, tgt, diff, ldd, part);
  check_launch("ce_eval");
  hipLaunchKernelGGL(ce_reduce_kernel, dim3(1), dim3(256), 0, st, part, nb, out);
  check_launch("ce_reduce");
}

}  // namespace eesen
