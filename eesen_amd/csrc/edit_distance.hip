// edit_distance.hip -- many Levenshtein distances at once, for gfx950 (INTEGRATION.md "Minimum Bayes risk").
//
// edit_distance_kernel computes what edit_distance() in ctc_host.cpp computes -- unit costs, the total only -- for a list of jobs.  A
// job is two spans (offset, length) of int32 tokens, the first into tok_a, the second into tok_b (often the same array); the result is
// one int32 per job.  Every integer equals the host's.
//
// One wavefront per job; no barrier between waves, no atomic.  The 64 lanes hold 64 consecutive columns of the DP table (tokens of the
// column sequence) and sweep the rows on the skewed schedule: at step k lane l owns cell (row k - l + 1, column j0 + l + 1).  "Up" is the
// lane's own last value, "left" lane l - 1's last value (one cross-lane move), "diagonal" the left of the step before.  The row
// sequence's token travels down the lanes in the same way, one lane per step.  Lane 0 takes its left and its row token from two
// registers of 64 that the wave refills every 64 steps.
// A column sequence of more than 64 tokens is taken in strips of 64 columns; a strip's right boundary column (one int per row) is
// carried in LDS, written by lane 63 and read 63 rows later by the next strip's refill -- in place, since the writes trail the reads.
// A strip costs rows + 63 steps, so of the two orientations the kernel takes the one with the smaller strips * (rows + 63).
#include "kernels.h"

namespace eesen {
namespace {

constexpr int kLanes = 64;

__device__ __forceinline__ long ed_cost(int rows, int cols) { return (long)((cols + kLanes - 1) / kLanes) * (rows + kLanes - 1); }

__global__ __launch_bounds__(256) void edit_distance_kernel(const int* __restrict__ tok_a, const int* __restrict__ tok_b, const int* __restrict__ jobs,
                                                            int njobs, int lds_ints, int* __restrict__ out) {
  extern __shared__ int ed_lds[];
  const int lane = threadIdx.x & (kLanes - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
  const int job = blockIdx.x * (blockDim.x / kLanes) + wave;
  if (job >= njobs) return;
  int* bnd = ed_lds + (size_t)wave * lds_ints;   // row i's value of the strip's right boundary column at bnd[i - 1]
  const int* jb = jobs + (size_t)job * 4;
  const int oa = jb[0], ob = jb[2];
  int m = jb[1], n = jb[3];
  if (m <= 0 || n <= 0) {
    if (lane == 0) out[job] = m > 0 ? m : n > 0 ? n : 0;
    return;
  }
  const int* __restrict__ a = tok_a + oa;   // rows
  const int* __restrict__ b = tok_b + ob;   // columns
  if (ed_cost(n, m) < ed_cost(m, n)) {      // (the distance is symmetric)
    const int* t = a; a = b; b = t;
    const int u = m; m = n; n = u;
  }
  if (m > lds_ints && n > kLanes) {         // (the launcher sizes the column for the longest sequence: never taken; -1 is no distance)
    if (lane == 0) out[job] = -1;
    return;
  }

  for (int j0 = 0; j0 < n; j0 += kLanes) {
    const int wl = min(kLanes, n - j0);     // columns of this strip
    const bool last = j0 + kLanes >= n;
    const int tb = lane < wl ? b[j0 + lane] : 0;
    int cur = j0 + lane + 1;                // D[i - 1][j]: row 0 of the table
    int diag = j0 + lane;                   // D[i - 1][j - 1]
    int ta = 0;
    const int nsteps = m + wl - 1;
    for (int k0 = 0; k0 < nsteps; k0 += kLanes) {
      const int r0 = k0 + lane;
      const int ac = r0 < m ? a[r0] : 0;
      int bc = r0 + 1;                      // D[i][0] = i
      if (j0 > 0) bc = r0 < m ? bnd[r0] : 0;
      __builtin_amdgcn_wave_barrier();      // (the refill's reads stay ahead of lane 63's writes below)
      const int kend = min(kLanes, nsteps - k0);
      for (int t = 0; t < kend; ++t) {
        const int a0 = __builtin_amdgcn_readlane(ac, t), l0 = __builtin_amdgcn_readlane(bc, t);
        const int up_cur = __shfl_up(cur, 1), up_ta = __shfl_up(ta, 1);
        const int left = lane == 0 ? l0 : up_cur;
        ta = lane == 0 ? a0 : up_ta;
        const int r = k0 + t - lane;        // row i = r + 1
        const bool active = (unsigned)r < (unsigned)m;
        const int nw = min(diag + (ta != tb ? 1 : 0), min(cur, left) + 1);
        if (active) { diag = left; cur = nw; }
        if (!last && lane == kLanes - 1 && active) bnd[r] = nw;
      }
      __builtin_amdgcn_wave_barrier();
    }
    if (last && lane == wl - 1) out[job] = cur;
  }
}

}  // namespace

void edit_distance_jobs(hipStream_t st, const int* tok_a, const int* tok_b, const int* jobs, int njobs, int max_len, int* out) {
  if (njobs <= 0) return;
  EESEN_REQUIRE(max_len >= 0 && max_len <= kEditDistanceMaxLen, EESEN_ERR_INVALID, "edit_distance_jobs: a sequence of more than 8192 tokens");
  const int lds_ints = std::max(max_len, 1);
  int waves = 4;   // as many as 64 KiB of boundary columns hold
  while (waves > 1 && (size_t)waves * lds_ints * sizeof(int) > 65536) waves >>= 1;
  hipLaunchKernelGGL(edit_distance_kernel, dim3(cdiv(njobs, waves)), dim3(waves * kLanes), (size_t)waves * lds_ints * sizeof(int), st, tok_a, tok_b, jobs,
                     njobs, lds_ints, out);
  check_launch("edit_distance_jobs");
}

}  // namespace eesen
