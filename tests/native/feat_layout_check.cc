// feat_layout_check.cc -- csrc/feat_layout.h alone, no HIP: the filterbank's and the pitch tracker's batch tables, their frame bounds,
// the front end's stage boundaries, paste-feats' row rule and the carving of the block that carries a batch's tables, against
// expectations written out by hand.  tests/test_feat_layout.py builds it under -fsanitize=address,undefined and runs it.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../eesen_amd/csrc/feat_layout.h"

namespace {

using namespace eesen;
int failures = 0;

void hold(bool ok, const char* what, long a = 0, long b = 0) {
  if (!ok) { std::printf("FAIL %s (%ld, %ld)\n", what, a, b); ++failures; }
}
template <class F>
bool refused(F f) {
  try { f(); } catch (const std::invalid_argument&) { return true; }
  return false;
}
template <class T>
void same(const char* what, const std::vector<T>& got, const std::vector<T>& want) {
  hold(got.size() == want.size(), what, (long)got.size(), (long)want.size());
  for (size_t i = 0; i < got.size() && i < want.size(); ++i) hold(got[i] == want[i], what, (long)i, (long)got[i]);
}

int frames_400_160(int n) { return n < 400 ? 0 : 1 + (n - 400) / 160; }   // 25 ms windows every 10 ms at 16 kHz, edges snipped

void fbank() {
  const int nsamp[3] = {0, 400, 1000};   // nothing, one frame exactly, four frames
  std::vector<long> off(3, -1), out_off(3, -1);
  std::vector<int> prefix(4, -1);
  const FbankTotals t = fbank_layout(nsamp, 3, 40, frames_400_160, off.data(), prefix.data(), out_off.data());
  same<long>("fbank: sample offsets", off, {0, 0, 400});
  same<int>("fbank: frame prefix", prefix, {0, 0, 1, 5});
  same<long>("fbank: output offsets", out_off, {0, 0, 40});
  hold(t.samp == 1400 && t.out == 200 && t.frames == 5, "fbank: totals", t.samp, t.out);
  const int neg[2] = {5, -1};
  hold(refused([&] { fbank_layout(neg, 2, 40, frames_400_160, off.data(), prefix.data(), out_off.data()); }), "fbank: a negative count is refused");

  // 80 utterances of 2^31 - 1 samples are 1 073 741 680 frames, below 2^30; one more is refused
  std::vector<int> big(81, 2147483647);
  std::vector<long> o(81), oo(81);
  std::vector<int> p(82);
  hold(frames_400_160(2147483647) == 13421771, "fbank: frames of 2^31 - 1 samples");
  const FbankTotals t80 = fbank_layout(big.data(), 80, 40, frames_400_160, o.data(), p.data(), oo.data());
  hold(t80.frames == 1073741680 && p[80] == 1073741680 && p[79] == 1073741680 - 13421771, "fbank: 80 long utterances pass", t80.frames);
  hold(t80.samp == 80L * 2147483647 && t80.out == 1073741680L * 40 && oo[79] == 79L * 13421771 * 40, "fbank: their totals", t80.samp, t80.out);
  hold(refused([&] { fbank_layout(big.data(), 81, 40, frames_400_160, o.data(), p.data(), oo.data()); }), "fbank: 81 are refused");
}

int fake_count(int n, int* f1, int* n1, int* n2) {   // a stand-in for PitchPlan::num_frames with numbers easy to follow
  *n2 = n / 4;
  *n1 = *n2 >= 2 ? *n2 - 2 : 0;
  *f1 = *n1 / 10;
  return *n2 / 10;
}

struct Row { long wave_off, down_off, proc_off; unsigned long long id; int nsamp, n1, n2, f1, frames, prefix; };
void utt_is(const char* what, const PitchUtt& u, const Row& r) {
  hold(u.wave_off == r.wave_off && u.down_off == r.down_off && u.proc_off == r.proc_off, what, u.wave_off, u.proc_off);
  hold(u.id == r.id && u.nsamp == r.nsamp && u.n1 == r.n1 && u.n2 == r.n2, what, (long)u.id, u.n2);
  hold(u.f1 == r.f1 && u.frames == r.frames && u.prefix == r.prefix && u.pad == 0, what, u.frames, u.prefix);
}

void pitch() {
  // counted from samples, delay 2, three processed columns, ids given
  const int nsamp[3] = {0, 100, 403};
  const unsigned long long ids[3] = {7, 9, 11};
  std::vector<PitchUtt> u(3);
  PitchTotals t = pitch_layout(nsamp, nullptr, ids, 1000, 3, 2, 3, fake_count, u.data());
  utt_is("pitch counted: utterance 0", u[0], {0, 0, 0, 7, 0, 0, 0, 0, 0, 0});
  utt_is("pitch counted: utterance 1", u[1], {0, 0, 0, 9, 100, 23, 25, 2, 2, 0});
  utt_is("pitch counted: utterance 2", u[2], {100, 25, 12, 11, 403, 98, 100, 9, 10, 2});
  hold(t.samp == 503 && t.down == 125 && t.proc == 48 && t.frames == 12, "pitch counted: totals", t.proc, t.frames);
  // the same with a first id
  t = pitch_layout(nsamp, nullptr, nullptr, 5, 3, 2, 3, fake_count, u.data());
  hold(u[0].id == 5 && u[1].id == 6 && u[2].id == 7 && u[2].proc_off == 12 && t.frames == 12, "pitch counted: ids from a first id");
  // frames given: no samples, the counting callable is not asked
  const int frames[3] = {3, 0, 4};
  auto never = [](int, int*, int*, int*) { hold(false, "pitch given: the frame count was asked for"); return 0; };
  t = pitch_layout(nullptr, frames, ids, 0, 3, 2, 3, never, u.data());
  utt_is("pitch given: utterance 0", u[0], {0, 0, 0, 7, 0, 0, 0, 0, 3, 0});
  utt_is("pitch given: utterance 1", u[1], {0, 0, 15, 9, 0, 0, 0, 0, 0, 3});
  utt_is("pitch given: utterance 2", u[2], {0, 0, 15, 11, 0, 0, 0, 0, 4, 3});
  hold(t.samp == 0 && t.down == 0 && t.proc == 33 && t.frames == 7, "pitch given: totals", t.proc, t.frames);
  t = pitch_layout(nullptr, frames, nullptr, 40, 3, 0, 1, never, u.data());
  hold(u[0].id == 40 && u[2].id == 42 && u[2].proc_off == 3 && t.proc == 7, "pitch given: ids from a first id, no delay");

  hold(kPitchMaxFrames == (1L << 28) && kPitchMaxStates == 1024, "pitch: the frame bound is 2^28");
  const int most[2] = {(1 << 28) - 1, 1};
  t = pitch_layout(nullptr, most, nullptr, 0, 1, 0, 1, never, u.data());
  hold(t.frames == (1L << 28) - 1, "pitch: 2^28 - 1 frames pass", t.frames);
  hold(refused([&] { pitch_layout(nullptr, most, nullptr, 0, 2, 0, 1, never, u.data()); }), "pitch: 2^28 frames are refused");
  const int neg[1] = {-1};
  hold(refused([&] { pitch_layout(nullptr, neg, nullptr, 0, 1, 0, 1, never, u.data()); }), "pitch: a negative frame count is refused");
  hold(refused([&] { pitch_layout(neg, nullptr, nullptr, 0, 1, 0, 1, fake_count, u.data()); }), "pitch: a negative sample count is refused");
}

void boundaries() {
  // splice(1, 1) -> subsample(n = 3, offset = 1) -> deltas(2, 2) on 4 columns; the one-frame utterance is empty behind the subsampling
  hold(subsample_frames(7, 3, 1) == 2 && subsample_frames(1, 3, 1) == 0 && subsample_frames(2, 3, 1) == 1 && subsample_frames(5, 3, 1) == 2 &&
       subsample_frames(6, 3, 0) == 2 && subsample_frames(7, 3, 0) == 3 && subsample_frames(4, -2, 0) == 8, "subsample_frames");
  const int frames[3] = {7, 1, 5}, dims[4] = {4, 12, 12, 36};
  std::vector<long> off(12, -1), total(4, -1);
  std::vector<int> fr(12, -1);
  auto stage = [](int k, int f) { return k == 1 ? subsample_frames(f, 3, 1) : f; };
  const int T = boundary_layout(frames, 3, dims, 4, stage, off.data(), fr.data(), total.data());
  same<int>("boundaries: frames", fr, {7, 1, 5, 7, 1, 5, 2, 0, 2, 2, 0, 2});
  same<long>("boundaries: offsets", off, {0, 28, 32, 0, 84, 96, 0, 24, 24, 0, 72, 72});
  same<long>("boundaries: totals", total, {52, 156, 48, 144});
  hold(T == 2, "boundaries: T", T);
  // no stage: one boundary; every utterance empty: T = 0, which the caller refuses
  std::vector<long> off1(2), total1(1);
  std::vector<int> fr1(2);
  const int two[2] = {3, 2}, none[2] = {0, 0}, neg[2] = {1, -2};
  hold(boundary_layout(two, 2, dims, 1, stage, off1.data(), fr1.data(), total1.data()) == 3 && off1[1] == 12 && total1[0] == 20, "boundaries: no stage");
  hold(boundary_layout(none, 2, dims, 1, stage, off1.data(), fr1.data(), total1.data()) == 0 && total1[0] == 0, "boundaries: an empty batch");
  hold(refused([&] { boundary_layout(neg, 2, dims, 1, stage, off1.data(), fr1.data(), total1.data()); }), "boundaries: a negative count is refused");
}

int paste(std::vector<int> frames, int tolerance) { return paste_frames(frames.data(), (int)frames.size(), tolerance); }
void pasting() {
  hold(paste({5, 5}, 0) == 5 && paste({5, 6}, 0) == 0 && paste({6, 5}, 0) == 0 && paste({9}, 0) == 9, "paste_frames: tolerance 0");
  hold(paste({5, 7}, 2) == 5 && paste({7, 5}, 2) == 5 && paste({5, 8}, 2) == 0 && paste({4, 6, 5}, 2) == 4 && paste({4, 6, 5, 7}, 2) == 0, "paste_frames: tolerance 2");
  hold(paste({0, 5}, 0) == 0 && paste({0, 2}, 2) == 0 && paste({2, 0}, 2) == 0 && paste({0, 0}, 0) == 0, "paste_frames: an empty input");
  const int one[1] = {1};
  hold(refused([&] { paste_frames(one, 0, 0); }), "paste_frames: no input is refused");
  hold(refused([&] { paste({1, 1}, -1); }), "paste_frames: a negative tolerance is refused");
  hold(refused([&] { paste({1, -1}, 0); }), "paste_frames: a negative count is refused");
}

// every table of the block starts on its own alignment, the tables follow one another without overlap, and the last byte of the last
// one is inside batch_words(); the block is allocated at exactly that size, so the sanitizer holds every write to it
void carving(int nb, int S, int head) {
  const size_t words = batch_words(nb, S, head);
  std::vector<long> block(words, 0);
  const BatchTables t = batch_carve(block.data(), nb, S, head);
  struct Seg { const char* what; void* p; size_t elem, n, align; };
  std::vector<Seg> segs = {{"off", t.off, 8, (size_t)nb * S, alignof(long)}};
  if (head) { segs.push_back({"fb_off", t.fb_off, 8, (size_t)S, alignof(long)}); segs.push_back({"ids", t.ids, 8, (size_t)S, alignof(unsigned long long)}); }
  if (head == kHeadFbankPitch) { segs.push_back({"utt", t.utt, sizeof(PitchUtt), (size_t)S, alignof(PitchUtt)}); segs.push_back({"proc_off", t.proc_off, 8, (size_t)S, alignof(long)}); }
  segs.push_back({"frames", t.frames, 4, (size_t)nb * S, alignof(int)});
  if (head) segs.push_back({"prefix", t.prefix, 4, (size_t)S + 1, alignof(int)});
  hold((head != kHeadNone) == (t.fb_off != nullptr) && (head != kHeadNone) == (t.ids != nullptr) && (head != kHeadNone) == (t.prefix != nullptr), "carve: the head's tables", head);
  hold((head == kHeadFbankPitch) == (t.utt != nullptr) && (head == kHeadFbankPitch) == (t.proc_off != nullptr), "carve: the pitch tables", head);
  char* at = reinterpret_cast<char*>(block.data());
  for (const Seg& g : segs) {
    hold(g.p != nullptr && reinterpret_cast<uintptr_t>(g.p) % g.align == 0, g.what, S, head);
    hold(static_cast<char*>(g.p) >= at, g.what, S, nb);             // behind the table before it
    at = static_cast<char*>(g.p) + g.elem * g.n;
  }
  const char* end = reinterpret_cast<char*>(block.data()) + words * 8;
  hold(at <= end && end - at < 8, "carve: the last byte is inside the block, and no word is spare", S, (long)(end - at));
  for (int i = 0; i < nb * S; ++i) { t.off[i] = 1; t.frames[i] = 2; }
  for (int s = 0; s < S && head; ++s) { t.fb_off[s] = 3; t.ids[s] = 4; t.prefix[s] = 5; }
  if (head) t.prefix[S] = 5;
  for (int s = 0; s < S && head == kHeadFbankPitch; ++s) { t.utt[s] = PitchUtt(); t.utt[s].pad = 6; t.proc_off[s] = 7; }
  bool kept = true;
  for (int i = 0; i < nb * S; ++i) kept = kept && t.off[i] == 1 && t.frames[i] == 2;
  for (int s = 0; s < S && head; ++s) kept = kept && t.fb_off[s] == 3 && t.ids[s] == 4 && t.prefix[s] == 5;
  for (int s = 0; s < S && head == kHeadFbankPitch; ++s) kept = kept && t.utt[s].pad == 6 && t.utt[s].wave_off == 0 && t.proc_off[s] == 7;
  hold(kept && (!head || t.prefix[S] == 5), "carve: no table overwrites another", S, head);
}

}  // namespace

int main() {
  fbank();
  pitch();
  boundaries();
  pasting();
  for (int S : {1, 2, 3, 4, 33})
    for (int nb : {1, 2, 4})
      for (int head : {kHeadNone, kHeadFbank, kHeadFbankPitch}) carving(nb, S, head);
  hold(batch_words(1, 1, kHeadNone) == 2 && batch_words(1, 2, kHeadNone) == 3 && batch_words(2, 3, kHeadFbank) == 12 + 5 &&
       batch_words(2, 3, kHeadFbankPitch) == 3 * (2 + 2 + 8 + 1) + 5 && sizeof(PitchUtt) == 64, "batch_words by hand");
  std::printf("%d failures\n", failures);
  return failures != 0;
}
