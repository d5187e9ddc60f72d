// ctc_layout.h -- where the CTC host code (ctc_host.cpp) keeps things: the buffers of a decode call, the padded length of a lattice,
// the blank-interleaved labels.  Host arithmetic only: no HIP and nothing of net.h, so tests/native/ctc_layout_check.cc compiles it alone.
#pragma once
#include <algorithm>
#include <cstddef>

namespace eesen {

enum DecodeMode { kDecodePlain = 0, kDecodeFused = 1, kDecodeWords = 2 };   // fused: token LM or spaced lexicon; words: unspaced lexicon

// The four device buffers of a decode call (Ctc::dec_f, dec_i, dec_trie, dec_out), offsets and totals in elements.  decode_batch
// carves them by this; decode_stamps, decode_rescore, decode_mbr and get_decode_candidates find what the last decode call left by
// the copy the Ctc keeps.  dec_out comes back to the host as one block (Ctc::decode_pin): its offsets hold on both sides.
struct DecodeLayout {
  int rows = 0, S = 0, T = 0, C = 0, B = 0, N = 0, mode = kDecodePlain;   // C = min(max_classes, K - 1); rows = 0: no decode call yet
  size_t n_cand = 0, n_beam = 0, n_trie = 0, NL = 0, n_hyp = 0;           // rows C, S B, S (1 + T B), S N, S N T
  // dec_f: candidate scores [rows][C], blank scores [rows], the final beam's scores [S][B] and (fused, words) LM sums [S][B]
  size_t csc = 0, sblank = 0, fscore = 0, flm = 0, n_f = 0;
  // dec_i: candidate ids [rows][C], frame counts [S], the final beam's nodes, lengths and (words) words, word counts [S][B], its sizes [S]
  size_t cid = 0, lens = 0, fnode = 0, flen = 0, fword = 0, fnw = 0, count = 0, n_i = 0;
  // dec_trie: every node's parent, its label and (words) the word closed in front of that label, n_trie each
  size_t trie[3] = {0, 0, 0}, n_t = 0;
  // dec_out: labels [NL][T], lengths [NL], scores [NL], (fused, words) LM sums [NL], (words) words and word ends [NL][T], word counts [NL]
  size_t hyp = 0, len = 0, score = 0, lmsum = 0, words = 0, ends = 0, wlen = 0, n_out = 0;
  bool fused() const { return mode != kDecodePlain; }
};

inline DecodeLayout decode_layout(int rows, int S, int K, int beam, int max_classes, int nbest, int mode) {
  DecodeLayout L;
  L.rows = rows; L.S = S; L.T = rows / S; L.C = std::min(max_classes, K - 1); L.B = beam; L.N = nbest; L.mode = mode;
  L.n_cand = (size_t)rows * L.C;
  L.n_beam = (size_t)S * beam;
  L.n_trie = (size_t)S * (1 + (size_t)L.T * beam);
  L.NL = (size_t)S * nbest;
  L.n_hyp = L.NL * L.T;
  const size_t lm = L.fused() ? 1 : 0, w = mode == kDecodeWords ? 1 : 0;   // a segment another mode has is empty here
  size_t o = 0;
  auto take = [&o](size_t n) { const size_t at = o; o += n; return at; };
  L.csc = take(L.n_cand); L.sblank = take(rows); L.fscore = take(L.n_beam); L.flm = take(lm * L.n_beam);
  L.n_f = o; o = 0;
  L.cid = take(L.n_cand); L.lens = take(S); L.fnode = take(L.n_beam); L.flen = take(L.n_beam); L.fword = take(w * L.n_beam);
  L.fnw = take(w * L.n_beam); L.count = take(S);
  L.n_i = o; o = 0;
  L.trie[0] = take(L.n_trie); L.trie[1] = take(L.n_trie); L.trie[2] = take(w * L.n_trie);
  L.n_t = o; o = 0;
  L.hyp = take(L.n_hyp); L.len = take(L.NL); L.score = take(L.NL); L.lmsum = take(lm * L.NL); L.words = take(w * L.n_hyp);
  L.ends = take(w * L.n_hyp); L.wlen = take(w * L.NL);
  L.n_out = o;
  return L;
}

// The padded length of the lattices of labellings of at most maxU labels: the power-of-two multiple of 64 that holds L' = 2 maxU + 1
// (ctc-loss.cc:118).  0 above 4096, that is beyond kMaxLatticeLabels labels: no sweep kernel takes those, the caller refuses or skips.
constexpr int kMaxLatticeLabels = 2047;
inline int lattice_pad(int maxU) {
  const long Lprime = 2L * maxU + 1;
  long Lpad = 64;
  while (Lpad < Lprime && Lpad <= 4096) Lpad *= 2;
  return Lpad <= 4096 ? (int)Lpad : 0;
}

// The labelling lab[0, U) as the lattice row lx[0, Lpad): blank, label, blank, ..., label, blank (ctc-loss.cc:116-129) and -1 behind.
// Returns the expanded length 2 U + 1.
inline int expand_labels(const int* lab, int U, int* lx, int Lpad) {
  for (int l = 0; l < U; ++l) { lx[2 * l] = 0; lx[2 * l + 1] = lab[l]; }
  lx[2 * U] = 0;
  std::fill(lx + 2 * U + 1, lx + Lpad, -1);
  return 2 * U + 1;
}

}  // namespace eesen
