// lm.h -- a token n-gram language model compiled to a deterministic backoff automaton (lm.cpp), and the view of its tables the
// fused prefix beam search reads on the device (ctc_decode.hip).  The computation: INTEGRATION.md "Decoding", "LM fusion".
#pragma once
#include <string>
#include <unordered_map>
#include <vector>

namespace eesen {

// what the text readers of lm.cpp and lex.cpp share: an error that carries the file and the line (0: none), the fields of a line,
// a non-negative decimal, and a units table (`symbol id` lines, ids in [1, K))
namespace text {
[[noreturn]] void fail(const std::string& path, long line, const std::string& what);
std::vector<std::string> fields_of(const std::string& s);
bool decimal(const std::string& s, long* v);
std::unordered_map<std::string, int> read_units(const char* path, int K);
}  // namespace text

// State 0 is the empty context and owns arcs [0, K-1): arc c-1 is class c.  Every other state's arcs are sorted by class id.
// lm_step(state, c): acc = 0; while the state has no arc for c: acc += bo_w[state], state = bo_next[state]; return (acc + w, next).
struct TokenLm {
  int K = 0, order = 0, start = 0;
  bool has_eos = false;
  unsigned long long serial = 0;   // unique per object: what a Ctc keys its device copy of the tables by
  std::vector<int> arc_off;        // [states + 1]
  std::vector<int> arc_cls, arc_next;
  std::vector<float> arc_w;
  std::vector<float> bo_w, fin;    // per state; fin = ln P(</s> | state), backoffs resolved (0 without </s>)
  std::vector<int> bo_next;
  std::vector<double> fin_abs;     // the absolute sum of the weights behind fin
  long long oov_dropped = 0;       // skip_oov: the n-grams left out because one of their words is outside the table

  // Fills this (fresh) object.  arpa: an ARPA file over token symbols; units: `symbol id` lines (ids in [1, K)), or null -- the words
  // are decimal class ids then.  skip_oov: an n-gram with a word that is neither in the table nor <s>, </s>, <unk> is dropped and
  // counted (after it has counted towards its section's header number) instead of being an error
  void from_arpa(const char* arpa, const char* units, int K, bool skip_oov = false);
  int states() const { return (int)bo_w.size(); }
  int arcs() const { return (int)arc_cls.size(); }
  int find_arc(int state, int c) const;                     // index of the state's arc for class c, or -1
  void step(int state, int c, float* w, int* next) const;   // fp32, the device's order of additions
  // ln P(labels [, </s>]) from the start state, accumulated in fp64 on the stored fp32 weights; abs_sum: the sum of their magnitudes
  double score(const int* labels, int n, bool eos, double* abs_sum) const;
};

// The tables on the device, packed so that a level of the walk is few dependent loads: state_rec holds {first arc, arc count, bo_next,
// bits of bo_w} per state (one 16-byte load), arc_wn {bits of w, next} per arc (one 8-byte load), arc_cls the sorted class ids.
struct LmTables {
  const int* state_rec;   // [states][4], 16-byte aligned
  const int* arc_wn;      // [arcs][2], 8-byte aligned
  const int* arc_cls;     // [arcs]
  const float* fin;       // [states]
  int start;
};

}  // namespace eesen
