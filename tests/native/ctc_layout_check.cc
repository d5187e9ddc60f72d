// ctc_layout_check.cc -- csrc/ctc_layout.h alone, no HIP: the buffers of a decode call in each of the three modes (segments in their
// order, contiguous, totals as written out here from the sizes), the padded lattice length at its edges, and the blank-interleaved
// labels against a row written out by hand.  tests/test_ctc_layout.py builds it under -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <vector>

#include "../../eesen_amd/csrc/ctc_layout.h"

namespace {

int failures = 0;

void hold(bool ok, const char* what, int a = 0, int b = 0) {
  if (!ok) { std::printf("FAIL %s (%d, %d)\n", what, a, b); ++failures; }
}

struct Seg { size_t at, n; };

// the segments follow one another from 0 without a gap or an overlap, and end at `total`
void chain(const char* what, const std::vector<Seg>& segs, size_t total, size_t want_total) {
  size_t o = 0;
  for (size_t i = 0; i < segs.size(); ++i) {
    hold(segs[i].at == o, what, (int)i, (int)segs[i].at);
    o += segs[i].n;
  }
  hold(o == total && total == want_total, what, (int)total, (int)want_total);
}

void layout(int rows, int S, int K, int beam, int max_classes, int nbest, int mode) {
  const eesen::DecodeLayout L = eesen::decode_layout(rows, S, K, beam, max_classes, nbest, mode);
  const bool fused = mode != eesen::kDecodePlain, words = mode == eesen::kDecodeWords;
  const size_t T = rows / S, C = max_classes < K - 1 ? max_classes : K - 1, SN = (size_t)S * nbest;
  const size_t n_cand = rows * C, n_beam = (size_t)S * beam, n_trie = S * (1 + T * beam), n_hyp = SN * T;
  hold(L.rows == rows && L.S == S && L.T == (int)T && L.C == (int)C && L.B == beam && L.N == nbest && L.mode == mode && L.fused() == fused, "shape", mode);
  hold(L.n_cand == n_cand && L.n_beam == n_beam && L.n_trie == n_trie && L.NL == SN && L.n_hyp == n_hyp, "sizes", mode);
  if (!words) {
    chain("floats", {{L.csc, n_cand}, {L.sblank, (size_t)rows}, {L.fscore, n_beam}, {L.flm, fused ? n_beam : 0}}, L.n_f,
          n_cand + rows + n_beam + (fused ? n_beam : 0));
    chain("ints", {{L.cid, n_cand}, {L.lens, (size_t)S}, {L.fnode, n_beam}, {L.flen, n_beam}, {L.fword, 0}, {L.fnw, 0}, {L.count, (size_t)S}}, L.n_i,
          n_cand + S + 2 * n_beam + S);
    chain("trie", {{L.trie[0], n_trie}, {L.trie[1], n_trie}, {L.trie[2], 0}}, L.n_t, 2 * n_trie);
    chain("out", {{L.hyp, n_hyp}, {L.len, SN}, {L.score, SN}, {L.lmsum, fused ? SN : 0}, {L.words, 0}, {L.ends, 0}, {L.wlen, 0}}, L.n_out,
          n_hyp + (fused ? 3 : 2) * SN);
  } else {
    chain("floats", {{L.csc, n_cand}, {L.sblank, (size_t)rows}, {L.fscore, n_beam}, {L.flm, n_beam}}, L.n_f, n_cand + rows + 2 * n_beam);
    chain("ints", {{L.cid, n_cand}, {L.lens, (size_t)S}, {L.fnode, n_beam}, {L.flen, n_beam}, {L.fword, n_beam}, {L.fnw, n_beam}, {L.count, (size_t)S}},
          L.n_i, n_cand + S + 4 * n_beam + S);
    chain("trie", {{L.trie[0], n_trie}, {L.trie[1], n_trie}, {L.trie[2], n_trie}}, L.n_t, 3 * n_trie);
    chain("out", {{L.hyp, n_hyp}, {L.len, SN}, {L.score, SN}, {L.lmsum, SN}, {L.words, n_hyp}, {L.ends, n_hyp}, {L.wlen, SN}}, L.n_out,
          3 * n_hyp + 4 * SN);
  }
}

}  // namespace

int main() {
  for (int mode : {eesen::kDecodePlain, eesen::kDecodeFused, eesen::kDecodeWords}) {
    layout(36, 3, 7, 4, 3, 2, mode);       // dense_3x12x7 as the decode tests call it
    layout(12, 1, 7, 4, 3, 1, mode);       // S = 1
    layout(36, 3, 7, 8, 6, 8, mode);       // nbest = beam
    layout(36, 3, 7, 16, 20, 3, mode);     // K - 1 < max_classes: six candidates per frame
    layout(480, 8, 46, 64, 32, 5, mode);   // the largest beam
    layout(2, 2, 2, 1, 1, 1, mode);        // one frame, one class beside the blank, beam 1
  }
  hold(eesen::decode_layout(36, 3, 7, 16, 20, 3, eesen::kDecodePlain).C == 6, "C = K - 1");

  hold(eesen::lattice_pad(0) == 64, "lattice_pad(0)", eesen::lattice_pad(0));
  hold(eesen::lattice_pad(31) == 64, "lattice_pad(31)", eesen::lattice_pad(31));          // L' = 63
  hold(eesen::lattice_pad(32) == 128, "lattice_pad(32)", eesen::lattice_pad(32));         // L' = 65
  hold(eesen::lattice_pad(2047) == 4096, "lattice_pad(2047)", eesen::lattice_pad(2047));  // L' = 4095
  hold(eesen::lattice_pad(2048) == 0, "lattice_pad(2048) is refused", eesen::lattice_pad(2048));
  hold(eesen::lattice_pad(1 << 30) == 0, "lattice_pad(2^30) is refused");
  hold(eesen::kMaxLatticeLabels == 2047, "kMaxLatticeLabels");

  const int lab[3] = {5, 5, 2};
  const int want[10] = {0, 5, 0, 5, 0, 2, 0, -1, -1, -1};
  std::vector<int> row(10, 77);   // exactly Lpad entries: the sanitizer holds the fill to them
  hold(eesen::expand_labels(lab, 3, row.data(), 10) == 7, "expand_labels: L'");
  for (int i = 0; i < 10; ++i) hold(row[i] == want[i], "expand_labels: row", i, row[i]);
  std::vector<int> one(1, 77);
  hold(eesen::expand_labels(nullptr, 0, one.data(), 1) == 1 && one[0] == 0, "expand_labels: the empty labelling");

  std::printf("%d failures\n", failures);
  return failures != 0;
}
