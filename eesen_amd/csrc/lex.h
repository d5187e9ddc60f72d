// lex.h -- a pronunciation lexicon over the net's own units compiled to a trie (lex.cpp), and the view of its tables the
// lexicon-constrained prefix beam search reads on the device (ctc_decode.hip).  The computation: INTEGRATION.md "Lexicon".
#pragma once
#include <string>
#include <vector>

namespace eesen {

struct TokenLm;

// Node 0 is the root.  Node v owns children [first[v], first[v] + count[v]) of child_cls (ascending class id) / child_node;
// word[v] is the id (1 .. V, in order of first appearance in the file) of the word whose spelling ends at v, or 0.
struct Lexicon {
  int K = 0, space = 0, max_word_len = 0;
  unsigned long long serial = 0;   // unique per object: what a Ctc keys its device copy of the tables by
  std::vector<std::string> names;  // [V + 1]; names[0] unused
  std::vector<int> first, count, word;     // per node
  std::vector<int> child_cls, child_node;  // per edge

  // Fills this (fresh) object.  path: `word unit unit ...` per spelling; units: `symbol id` lines, or null -- the units are decimal
  // class ids then
  void from_file(const char* path, const char* units, int K, int space);

  // The unspaced kind (INTEGRATION.md "Words without a boundary unit"): no boundary unit (space = 0, the blank's id) and several
  // words per spelling.  words(v) = node_words[wfirst[v] .. wfirst[v] + wcount[v]), ascending ids; word[v] is its smallest or 0.
  // At most kMaxHomophones words per spelling: a successor's slot (0 inside, 1 + i closing the i-th word) is four bits of the
  // search's tie index, and so is a final hypothesis' word index.
  static constexpr int kMaxHomophones = 15;
  bool unspaced = false;
  int max_homophones = 0;                      // H: the largest words(v)
  std::vector<int> wfirst, wcount, node_words;
  void from_file_unspaced(const char* path, const char* units, int K);
  int V() const { return (int)names.size() - 1; }
  int nodes() const { return (int)word.size(); }
  int child(int node, int c) const;   // the child of `node` for class c, or -1
  // segments a labelling of L = {empty} + {w1 Sp w2 ... Sp wn}: the word ids into out (room for (n + 1) / 2), their number into
  // *num; false for a labelling outside L
  bool words(const int* labels, int n, int* out, int* num) const;
  void write_words(const char* path) const;   // `word id` lines: the units table of a word LM with K = V + 1
  // The unigram look-ahead table of a word LM over this lexicon (lm.K == V + 1; INTEGRATION.md "LM look-ahead"): out [nodes],
  // out[v] = max of lm.step(0, w) over the words w whose spelling passes through or ends at v, by comparisons only
  void lookahead(const TokenLm& lm, float* out) const;
 private:
  void compile(const char* path, const char* units);
};

// The tables on the device: node_rec holds {first child, child count, word, 0} per node (one 16-byte load), child_cls the sorted
// class ids of the edges and child_node their targets.
struct LexTables {
  const int* node_rec;    // [nodes][4], 16-byte aligned
  const int* child_cls;   // [edges]
  const int* child_node;  // [edges]
  int space;
};

// The unspaced kind's tables: node_rec holds {first child, child count, first word slot, word count} per node, node_words the word
// ids of every node's list, H the largest list.
struct WordLexTables {
  const int* node_rec;    // [nodes][4], 16-byte aligned
  const int* child_cls;   // [edges]
  const int* child_node;  // [edges]
  const int* node_words;  // [sum of the word counts]
  int H, K;
};

}  // namespace eesen
