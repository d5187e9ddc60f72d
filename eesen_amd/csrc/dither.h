// dither.h -- the counter-based normal generator behind the filterbank's dither (fbank.hip) and the pitch post-processing's
// delta-pitch noise (pitch.hip): a draw is a pure function of its key and two counters, so a seed reproduces its output.
#pragma once
#include <hip/hip_runtime.h>

namespace eesen {

// splitmix64's finaliser
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// one standard normal per (key, frame, sample): Box-Muller on two 24-bit uniforms of one 64-bit word
__device__ __forceinline__ float dither_gauss(unsigned long long key, int frame, int sample) {
  const unsigned long long h = mix64(key + (((unsigned long long)(unsigned)frame << 32) | (unsigned)sample));
  const float u1 = (float)((unsigned)(h >> 40) + 1u) * 5.9604644775390625e-8f;   // (0, 1]
  const float u2 = (float)((unsigned)h & 0xFFFFFFu) * 5.9604644775390625e-8f;    // [0, 1)
  return sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
}

}  // namespace eesen
