// feat_layout.h -- how a batch of the feature path is laid out: the filterbank's and the pitch tracker's per-utterance tables, the
// front end's stage boundaries, paste-feats' row rule, and the one block of 8-byte words that carries a batch's tables to the device.
// Host arithmetic only: no HIP, no plan (frame counts come in as callables), and no sample pointers -- a batch is refused on its
// counts alone, before anything of it is read.  A refusal is a std::invalid_argument, which the C-ABI's guard turns into
// EESEN_ERR_INVALID.  The stand-alone extractors write these tables into vectors, the feeder into a slot's pinned block;
// tests/native/feat_layout_check.cc compiles this file alone.
#pragma once
#include <algorithm>
#include <cstddef>
#include <stdexcept>

namespace eesen {

inline void layout_require(bool ok, const char* msg) { if (!ok) throw std::invalid_argument(msg); }

// The noise key of utterance s: the caller's, or counted on from `first`.
inline unsigned long long key_of(const unsigned long long* ids, unsigned long long first, int s) { return ids ? ids[s] : first + s; }

// ---- filterbank: off[s] samples and prefix[s] frames in front of utterance s (prefix[S]: all frames), out_off[s] floats in front of
// its [frames x dim] matrix.  The kernel numbers a launch's frames in 30 bits.
struct FbankTotals { long samp = 0, out = 0; int frames = 0; };
template <class Frames>   // frames_of(nsamp) -> frames
FbankTotals fbank_layout(const int* nsamp, int S, int dim, Frames frames_of, long* off, int* prefix, long* out_off) {
  FbankTotals t;
  long frames = 0;
  for (int s = 0; s < S; ++s) {
    layout_require(nsamp[s] >= 0, "negative sample count");
    off[s] = t.samp;
    prefix[s] = (int)frames;
    out_off[s] = t.out;
    const int f = frames_of(nsamp[s]);
    t.samp += nsamp[s];
    t.out += (long)f * dim;
    frames += f;
    layout_require(frames < (1L << 30), "too many frames in one batch");
  }
  t.frames = prefix[S] = (int)frames;
  return t;
}

// ---- pitch: one utterance of a launch, as the kernels see it.
struct PitchUtt {
  long wave_off, down_off;       // into the packed samples / down-sampled samples
  long proc_off;                 // floats in front of its processed matrix
  unsigned long long id;
  int nsamp, n1, n2;
  int f1, frames, prefix;        // prefix: frames in front of it in the launch
  int pad;
};
constexpr int kPitchMaxStates = 1024;        // search kernel: one thread per lag state, one workgroup per utterance
constexpr long kPitchMaxFrames = (1L << 30) / kPitchMaxStates * 256;   // frames of one launch: [frames x states] offsets stay below 2^38
struct PitchTotals { long samp = 0, down = 0, proc = 0, frames = 0; };
// frames[s] given (post-processing alone: no samples) or counted from nsamp[s] by count(nsamp, &f1, &n1, &n2); a processed matrix has
// frames + delay rows of proc_dim floats, none without a frame
template <class Count>
PitchTotals pitch_layout(const int* nsamp, const int* frames, const unsigned long long* ids, unsigned long long first_id, int S, int delay,
                         int proc_dim, Count count, PitchUtt* utt) {
  PitchTotals t;
  for (int s = 0; s < S; ++s) {
    PitchUtt u = PitchUtt();
    if (frames) {
      layout_require(frames[s] >= 0, "negative frame count");
      u.frames = frames[s];
    } else {
      layout_require(nsamp[s] >= 0, "negative sample count");
      u.nsamp = nsamp[s];
      u.frames = count(nsamp[s], &u.f1, &u.n1, &u.n2);
    }
    u.wave_off = t.samp; u.down_off = t.down; u.proc_off = t.proc;
    u.prefix = (int)t.frames;
    u.id = key_of(ids, first_id, s);
    utt[s] = u;
    t.samp += u.nsamp;
    t.down += u.n2;
    t.proc += u.frames ? (long)(u.frames + delay) * proc_dim : 0;
    t.frames += u.frames;
    layout_require(t.frames < kPitchMaxFrames, "too many frames in one batch");
  }
  return t;
}

// ---- the front end's stage boundaries: boundary 0 is what was submitted, boundary b what stage b - 1 wrote.  Utterance s holds
// fr[b * S + s] frames of dims[b] floats at boundary b, off[b * S + s] floats in front of it; total[b] floats in all.  Returns T, the
// longest utterance at the last boundary.
inline int subsample_frames(int T, int n, int offset) {   // subsample-feats.cc:82-84: the k = offset, offset + n, ... < T; n < 0 repeats
  if (n < 0) return T * (-n);
  return T > offset ? (T - offset + n - 1) / n : 0;
}
template <class StageFrames>   // stage_frames(k, frames in) -> frames out of stage k
int boundary_layout(const int* frames, int S, const int* dims, int nb, StageFrames stage_frames, long* off, int* fr, long* total) {
  std::fill(total, total + nb, 0L);
  int T = 0;
  for (int s = 0; s < S; ++s) {
    layout_require(frames[s] >= 0, "negative frame count");
    int f = frames[s];
    for (int b = 0; b < nb; ++b) {
      if (b) f = stage_frames(b - 1, f);
      off[(size_t)b * S + s] = total[b];
      fr[(size_t)b * S + s] = f;
      total[b] += (long)f * dims[b];
    }
    T = std::max(T, f);
  }
  return T;
}

// AppendFeats' length rule (src/featbin/paste-feats.cc:35-56) on row counts alone: the shortest input's rows, or none when the
// longest exceeds it by more than the tolerance or an input is empty.  The feeder's combined head, eesen_paste_feats and the tools
// all decide through this one function.
inline int paste_frames(const int* frames, int n_inputs, int tolerance) {
  layout_require(n_inputs >= 1, "paste-feats: need at least one input");
  layout_require(tolerance >= 0, "paste-feats: --length-tolerance must not be negative");
  int min_len = frames[0], max_len = frames[0];
  for (int i = 0; i < n_inputs; ++i) {
    layout_require(frames[i] >= 0, "negative frame count");
    min_len = std::min(min_len, frames[i]);
    max_len = std::max(max_len, frames[i]);
  }
  return (max_len - min_len > tolerance || min_len == 0) ? 0 : min_len;
}

// ---- the tables of one batch in one block of 8-byte words: one pinned block and one device block per staging slot, one upload.
// The 8-byte tables first, the ints behind them.  The same carving gives the host view and the device view.
enum HeadKind { kHeadNone = 0, kHeadFbank = 1, kHeadFbankPitch = 2 };
struct BatchTables {
  long* off; int* frames;          // [nb x S] each: the stage boundaries
  // a head stage only, [S] each: the filterbank's output offsets and noise keys, its frame prefix [S + 1]; the combined head also
  // the PitchUtt table and the processed pitch matrices' offsets (paste-feats reads them as a table of their own)
  long* fb_off; unsigned long long* ids; int* prefix;
  PitchUtt* utt; long* proc_off;
};
static_assert(sizeof(PitchUtt) % 8 == 0 && sizeof(long) == 8, "the tables are laid out in 8-byte words");
inline size_t batch_words(int nb, int S, int head) {
  const size_t ints = (size_t)nb * S + (head ? (size_t)S + 1 : 0);
  return (size_t)S * (nb + (head ? 2 : 0) + (head == kHeadFbankPitch ? sizeof(PitchUtt) / 8 + 1 : 0)) + (ints + 1) / 2;
}
inline BatchTables batch_carve(void* base, int nb, int S, int head) {
  BatchTables t = BatchTables();
  long* w = static_cast<long*>(base);
  auto take = [&w](size_t n) { long* at = w; w += n; return at; };
  t.off = take((size_t)nb * S);
  if (head) { t.fb_off = take(S); t.ids = reinterpret_cast<unsigned long long*>(take(S)); }
  if (head == kHeadFbankPitch) { t.utt = reinterpret_cast<PitchUtt*>(take((size_t)S * (sizeof(PitchUtt) / 8))); t.proc_off = take(S); }
  t.frames = reinterpret_cast<int*>(w);
  if (head) t.prefix = t.frames + (size_t)nb * S;
  return t;
}

}  // namespace eesen
