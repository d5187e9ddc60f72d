// lex.cpp -- lexicon file -> trie over the net's own units (the shape of an L.fst without OpenFst, for systems whose words are
// separated by a space unit).  Host code only.  The rules are INTEGRATION.md's "Lexicon": one `word unit unit ...` line per spelling,
// units resolved through the units table or as decimal class ids, word ids 1 .. V in order of first appearance.
#include <atomic>
#include <fstream>
#include <map>
#include <unordered_map>

#include "common.h"
#include "lex.h"
#include "lm.h"

namespace eesen {

using namespace text;

void Lexicon::from_file(const char* path, const char* units, int K_, int space_) {
  EESEN_REQUIRE(K_ >= 3, EESEN_ERR_INVALID, "a lexicon needs the blank, the space and at least one other class (K >= 3)");
  EESEN_REQUIRE(space_ >= 1 && space_ < K_, EESEN_ERR_INVALID, "the space class must lie in [1, K)");
  K = K_;
  space = space_;
  unspaced = false;
  compile(path, units);
}

void Lexicon::from_file_unspaced(const char* path, const char* units, int K_) {
  EESEN_REQUIRE(K_ >= 2, EESEN_ERR_INVALID, "an unspaced lexicon needs the blank and at least one other class (K >= 2)");
  K = K_;
  space = 0;   // the blank's id: no unit can be it
  unspaced = true;
  compile(path, units);
}

void Lexicon::compile(const char* path, const char* units) {
  const bool have_units = units != nullptr && units[0] != 0;
  std::unordered_map<std::string, int> table;
  if (have_units) table = read_units(units, K);
  std::ifstream in(path);
  if (!in) fail(path, 0, "cannot open the lexicon");
  names.assign(1, std::string());
  std::vector<std::vector<std::pair<int, long>>> ends(1);   // unspaced, per node: (word, the line that put it there), ascending
  std::unordered_map<std::string, int> id_of;
  std::vector<std::map<int, int>> kids(1);   // per node: class -> child (ordered: the children come out sorted)
  word.assign(1, 0);
  std::string line;
  for (long ln = 1; std::getline(in, line); ++ln) {
    const auto f = fields_of(line);
    if (f.empty()) continue;
    if (f.size() == 1) fail(path, ln, "word " + f[0] + " has an empty spelling");
    std::vector<int> sp;
    for (size_t i = 1; i < f.size(); ++i) {
      long id = 0;
      if (have_units) {
        const auto it = table.find(f[i]);
        if (it == table.end()) fail(path, ln, "unit " + f[i] + " is not in the units table");
        id = it->second;
      } else if (!decimal(f[i], &id)) {
        fail(path, ln, "unit " + f[i] + " is no decimal class id");
      }
      if (id < 1 || id >= K) fail(path, ln, "unit " + f[i] + " outside [1, K) with K = " + std::to_string(K));
      if (!unspaced && id == space) fail(path, ln, "unit " + f[i] + " is the space class: a spelling cannot hold it");
      sp.push_back((int)id);
    }
    int v = 0;
    for (int c : sp) {
      const auto it = kids[v].find(c);
      if (it != kids[v].end()) { v = it->second; continue; }
      if (kids.size() >= ((size_t)1 << 30)) fail(path, ln, "the trie must stay below 2^30 nodes");
      const int made = (int)kids.size();
      kids[v].emplace(c, made);
      kids.emplace_back();
      word.push_back(0);
      if (unspaced) ends.emplace_back();
      v = made;
    }
    // (the word takes its id only now: a line that fails leaves no word behind)
    const auto known = id_of.find(f[0]);
    const int w = known != id_of.end() ? known->second : (int)names.size();
    if (unspaced) {
      auto& e = ends[v];
      auto at = std::lower_bound(e.begin(), e.end(), std::make_pair(w, 0L));
      if (at == e.end() || at->first != w) {
        if ((int)e.size() >= kMaxHomophones)
          fail(path, ln, "word " + f[0] + " is one more than " + std::to_string(kMaxHomophones) + " words with the same spelling (the first of them: " +
                             names[e.front().first] + ", line " + std::to_string(e.front().second) + ")");
        e.insert(at, std::make_pair(w, ln));
      }
    } else if (word[v] != 0 && word[v] != w) fail(path, ln, "words " + names[word[v]] + " and " + f[0] + " have the same spelling: a labelling would not determine the word");
    if (known == id_of.end()) { id_of.emplace(f[0], w); names.push_back(f[0]); }
    word[v] = unspaced ? ends[v].front().first : w;
    max_word_len = std::max(max_word_len, (int)sp.size());
  }
  if (V() < 1) fail(path, 0, "the lexicon holds no word");
  const int n = (int)kids.size();
  first.assign(n, 0);
  count.assign(n, 0);
  for (int v = 0; v < n; ++v) {
    first[v] = (int)child_cls.size();
    count[v] = (int)kids[v].size();
    for (const auto& kv : kids[v]) { child_cls.push_back(kv.first); child_node.push_back(kv.second); }
  }
  if (unspaced) {
    wfirst.assign(n, 0);
    wcount.assign(n, 0);
    for (int v = 0; v < n; ++v) {
      wfirst[v] = (int)node_words.size();
      wcount[v] = (int)ends[v].size();
      for (const auto& e : ends[v]) node_words.push_back(e.first);
      max_homophones = std::max(max_homophones, wcount[v]);
    }
  }
  static std::atomic<unsigned long long> next_serial{1};
  serial = next_serial++;
}

int Lexicon::child(int node, int c) const {
  EESEN_REQUIRE(node >= 0 && node < nodes(), EESEN_ERR_INVALID, "lexicon node out of range");
  const int* lo = child_cls.data() + first[node];
  const int* hi = lo + count[node];
  const int* it = std::lower_bound(lo, hi, c);
  return it != hi && *it == c ? child_node[it - child_cls.data()] : -1;
}

bool Lexicon::words(const int* labels, int n, int* out, int* num) const {
  EESEN_REQUIRE(!unspaced, EESEN_ERR_INVALID, "an unspaced lexicon does not segment a labelling (the segmentation is ambiguous): the words come from eesen_ctc_decode_parallel_words");
  int v = 0, nw = 0;
  for (int i = 0; i < n; ++i) {
    const int c = labels[i];
    if (c == space) {
      if (word[v] == 0) return false;   // (the root has no word: a leading or a double space)
      out[nw++] = word[v];
      v = 0;
    } else {
      if (c < 1 || c >= K) return false;
      v = child(v, c);
      if (v < 0) return false;
    }
  }
  if (n > 0) {
    if (word[v] == 0) return false;     // mid-word, or a trailing space
    out[nw++] = word[v];
  }
  *num = nw;
  return true;
}

void Lexicon::lookahead(const TokenLm& lm, float* out) const {
  EESEN_REQUIRE(lm.K == V() + 1, EESEN_ERR_INVALID, "the word LM's K must be the lexicon's word count + 1 (build it over eesen_lex_write_words' table)");
  const int n = nodes();
  // a child's id is above its parent's (compile() makes a node behind its parent), so one descending pass is bottom-up
  for (int v = n - 1; v >= 0; --v) {
    bool have = false;
    float best = 0.f;
    auto take = [&](float u) { if (!have || u > best) best = u; have = true; };
    auto unigram = [&](int w) { float u; int next; lm.step(0, w, &u, &next); return u; };
    if (unspaced) for (int i = 0; i < wcount[v]; ++i) take(unigram(node_words[wfirst[v] + i]));
    else if (word[v] != 0) take(unigram(word[v]));
    for (int e = first[v]; e < first[v] + count[v]; ++e) take(out[child_node[e]]);
    out[v] = best;   // (every node has a word at or below it: a leaf ends a spelling)
  }
}

void Lexicon::write_words(const char* path) const {
  std::ofstream out(path);
  for (int w = 1; w <= V(); ++w) out << names[w] << ' ' << w << '\n';
  out.close();
  if (!out) throw Error(EESEN_ERR_IO, std::string(path) + ": cannot write the words table");
}

}  // namespace eesen
