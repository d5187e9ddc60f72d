// cmvn_stats.h -- what the two callers of the CMVN statistics kernel (cmvn_stats.hip: the stand-alone call and the feeder's tap) share:
// the row chunking, the room the partial sums need, and the launch.
#pragma once
#include "common.h"

namespace eesen {

constexpr int kCmvnThreads = 256;
// Rows of one workgroup.  A workgroup covers min(D, 256) columns at a time with 256 / min(D, 256) rows side by side, and walks at most
// 32 such passes per column tile: 160 rows at D = 43, 64 at D = 120, 32 from D = 129 on.  A function of D alone, so where an
// utterance's chunks begin depends on nothing but its own frame count.
inline int cmvn_chunk_rows(int D) { return 32 * std::max(1, kCmvnThreads / std::min(D, kCmvnThreads)); }
inline int cmvn_chunks(int frames, int chunk_rows) { return (frames + chunk_rows - 1) / chunk_rows; }
// Utterance s, with P rows in front of it in the batch, owns the partial matrices P / chunk_rows + s onwards: the ranges of two
// neighbours never meet (floor(P / R) + ceil(f / R) <= floor((P + f) / R) + 1), and no table of chunk offsets has to go up.
inline size_t cmvn_partial_doubles(long total_rows, int S, int D, int chunk_rows) {
  return ((size_t)(total_rows / chunk_rows) + (size_t)S + 1) * 2 * ((size_t)D + 1);
}
// stats[S][2][D + 1] of the packed batch x (off[s] floats in front of utterance s, frames[s] rows of D floats); w: NULL, or one weight
// per row of the batch, in the rows' order.  Two launches: partial sums per chunk of chunk_rows rows (cmvn_chunk_rows(D)) into
// `partials` (cmvn_partial_doubles), and their sum in chunk order.  max_frames: the longest utterance.
void cmvn_stats_launch(const float* x, const long* off, const int* frames, const float* w, int S, int D, int max_frames, int chunk_rows,
                       double* partials, double* stats, hipStream_t st);

}  // namespace eesen
