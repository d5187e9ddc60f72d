// lm.cpp -- ARPA file -> deterministic backoff automaton over the net's own tokens (the shape of a G.fst, without OpenFst).  Host
// code only.  The rules are INTEGRATION.md's "LM fusion": words resolve through the units table first, then <s>, </s> and <unk>;
// values are log10 in the file and float(v * ln 10) here; the file need not be suffix-closed.
#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <tuple>
#include <unordered_map>

#include "common.h"
#include "lm.h"

namespace eesen {
namespace text {

[[noreturn]] void fail(const std::string& path, long line, const std::string& what) {
  throw Error(EESEN_ERR_INVALID, path + (line > 0 ? ":" + std::to_string(line) : std::string()) + ": " + what);
}

std::vector<std::string> fields_of(const std::string& s) {
  std::vector<std::string> f;
  std::istringstream in(s);
  for (std::string w; in >> w;) f.push_back(w);
  return f;
}

bool decimal(const std::string& s, long* v) {
  if (s.empty() || s.size() > 18) return false;   // (fits a long; the limits are checked where the number is used)
  for (char ch : s)
    if (ch < '0' || ch > '9') return false;
  *v = std::strtol(s.c_str(), nullptr, 10);
  return true;
}

std::unordered_map<std::string, int> read_units(const char* path, int K) {
  std::ifstream in(path);
  if (!in) fail(path, 0, "cannot open the units table");
  std::unordered_map<std::string, int> u;
  std::string line;
  for (long ln = 1; std::getline(in, line); ++ln) {
    const auto f = fields_of(line);
    if (f.empty()) continue;
    long id = 0;
    if (f.size() != 2 || !decimal(f[1], &id)) fail(path, ln, "a units line is `symbol id`");
    if (id < 1 || id >= K) fail(path, ln, "unit id " + f[1] + " outside [1, K) with K = " + std::to_string(K));
    if (!u.emplace(f[0], (int)id).second) fail(path, ln, "unit " + f[0] + " listed twice");
  }
  return u;
}

}  // namespace text

namespace {

using namespace text;
constexpr int kMaxOrder = 8;
constexpr double kLn10 = 2.302585092994045684;
using Gram = std::vector<int>;
struct Entry { float w = 0.f, bo = 0.f; int state = -1; };

bool number(const std::string& s, double* v) {
  char* end = nullptr;
  errno = 0;
  *v = std::strtod(s.c_str(), &end);
  return end != s.c_str() && *end == 0 && std::isfinite(*v);
}

}  // namespace

void TokenLm::from_arpa(const char* arpa, const char* units, int K, bool skip_oov) {
  EESEN_REQUIRE(K >= 2, EESEN_ERR_INVALID, "a token LM needs the blank and at least one other class (K >= 2)");
  const int BOS = K, EOS = K + 1, UNK = K + 2;
  const bool have_units = units != nullptr && units[0] != 0;
  std::unordered_map<std::string, int> table;
  if (have_units) table = read_units(units, K);
  std::ifstream in(arpa);
  if (!in) fail(arpa, 0, "cannot open the ARPA file");
  auto resolve = [&](const std::string& w, long ln) -> int {
    if (have_units) {
      const auto it = table.find(w);
      if (it != table.end()) return it->second;
    } else {
      long id = 0;
      if (decimal(w, &id)) {
        if (id < 1 || id >= K) {
          if (skip_oov) return -1;
          fail(arpa, ln, "word " + w + " is no class id in [1, K) with K = " + std::to_string(K));
        }
        return (int)id;
      }
    }
    if (w == "<s>") return BOS;
    if (w == "</s>") return EOS;
    if (w == "<unk>") return UNK;
    if (skip_oov) return -1;
    fail(arpa, ln, "word " + w + (have_units ? " is neither a unit nor <s>, </s>, <unk>" : " is neither a decimal class id nor <s>, </s>, <unk>"));
  };

  // ---- the file
  std::string line;
  long ln = 0;
  bool data = false;
  while (std::getline(in, line)) {
    ++ln;
    const auto f = fields_of(line);
    if (f.size() == 1 && f[0] == "\\data\\") { data = true; break; }
  }
  if (!data) fail(arpa, 0, "no \\data\\ section");
  std::vector<long> counts;   // counts[n - 1]
  bool have_line = false;
  while (std::getline(in, line)) {
    ++ln;
    const auto f = fields_of(line);
    if (f.empty()) continue;
    if (f[0] != "ngram") { have_line = true; break; }
    // `ngram n=count`
    std::string rest;
    for (size_t i = 1; i < f.size(); ++i) rest += f[i];
    const size_t eq = rest.find('=');
    long n = 0, cnt = 0;
    if (eq == std::string::npos || !decimal(rest.substr(0, eq), &n) || !decimal(rest.substr(eq + 1), &cnt)) fail(arpa, ln, "a header line is `ngram n=count`");
    if (n != (long)counts.size() + 1) fail(arpa, ln, "the header lists order " + std::to_string(n) + " out of sequence");
    if (cnt >= (1l << 31)) throw Error(EESEN_ERR_INVALID, std::string(arpa) + ": states and arcs must stay below 2^31");
    if (n > kMaxOrder) throw Error(EESEN_ERR_INVALID, std::string(arpa) + ": order " + std::to_string(n) + " above the limit of " + std::to_string(kMaxOrder) + " (order 1..8)");
    counts.push_back(cnt);
  }
  const int N = (int)counts.size();
  if (N < 1) throw Error(EESEN_ERR_INVALID, std::string(arpa) + ": the header lists no order (order 1..8)");
  long long total = 0;
  for (long c : counts) total += c;
  if (total >= (1ll << 31)) throw Error(EESEN_ERR_INVALID, std::string(arpa) + ": states and arcs must stay below 2^31");

  std::vector<std::map<Gram, Entry>> grams(N + 1);   // grams[n]: the n-grams
  int section = 0;
  long seen = 0;
  auto close_section = [&]() {
    if (section > 0 && seen != counts[section - 1])
      fail(arpa, ln, "section \\" + std::to_string(section) + "-grams: holds " + std::to_string(seen) + " n-grams, the header says " + std::to_string(counts[section - 1]));
  };
  bool ended = false;
  for (; have_line || std::getline(in, line); have_line = false) {
    if (!have_line) ++ln;
    const auto f = fields_of(line);
    if (f.empty()) continue;
    if (f.size() == 1 && f[0] == "\\end\\") { ended = true; break; }
    if (f.size() == 1 && f[0].size() > 8 && f[0][0] == '\\' && f[0].compare(f[0].size() - 7, 7, "-grams:") == 0) {
      long n = 0;
      if (!decimal(f[0].substr(1, f[0].size() - 8), &n) || n != section + 1 || n > N) fail(arpa, ln, "section " + f[0] + " out of sequence");
      close_section();
      section = (int)n;
      seen = 0;
      continue;
    }
    if (section == 0) fail(arpa, ln, "an n-gram line before any \\n-grams: section");
    const int n = section;
    if (!((int)f.size() == n + 1 || ((int)f.size() == n + 2 && n < N)))
      fail(arpa, ln, "a line of the " + std::to_string(n) + "-grams needs a value, " + std::to_string(n) + " words" + (n < N ? " and at most a backoff weight" : ""));
    double v = 0, b = 0;
    if (!number(f[0], &v)) fail(arpa, ln, "value " + f[0] + " is not a finite number");
    if ((int)f.size() == n + 2 && !number(f[n + 1], &b)) fail(arpa, ln, "backoff weight " + f[n + 1] + " is not a finite number");
    Gram g(n);
    bool oov = false;
    for (int i = 0; i < n; ++i) oov |= (g[i] = resolve(f[1 + i], ln)) < 0;
    if (oov) {   // skip_oov: counted towards its section, then dropped (as are, by the same rule, all n-grams that extend it)
      ++seen;
      ++oov_dropped;
      continue;
    }
    if (n > 1 && !grams[n - 1].count(Gram(g.begin(), g.end() - 1))) fail(arpa, ln, "the " + std::to_string(n - 1) + "-word prefix of this n-gram is not listed");
    Entry e;
    e.w = (float)(v * kLn10);
    e.bo = (float)(b * kLn10);
    if (!grams[n].emplace(std::move(g), e).second) fail(arpa, ln, "this n-gram is listed twice");
    ++seen;
  }
  (void)ended;   // (a file that stops after its last section is complete if the counts agree)
  close_section();
  if (section != N) fail(arpa, ln, "the header announces " + std::to_string(N) + " orders, the file holds " + std::to_string(section) + " sections");

  // ---- coverage: every class has a unigram, its own or <unk>'s
  const auto unk = grams[1].find(Gram{UNK});
  for (int c = 1; c < K; ++c)
    if (!grams[1].count(Gram{c}) && unk == grams[1].end()) {
      std::string name;   // with a table, what the file would have called it (a word of a 20 000-word lexicon is not found by its id)
      for (const auto& kv : table)
        if (kv.second == c) name = " (" + kv.first + ")";
      throw Error(EESEN_ERR_INVALID, std::string(arpa) + ": class " + std::to_string(c) + name + " has no unigram and the file has no <unk>");
    }

  // ---- states: the empty context, then every n-gram of order < N that does not end in </s> or <unk>
  TokenLm* lm = this;
  static std::atomic<unsigned long long> next_serial{1};
  lm->serial = next_serial++;
  lm->K = K;
  lm->order = N;
  int ns = 1;
  for (int n = 1; n < N; ++n)
    for (auto& kv : grams[n])
      if (kv.first.back() != EOS && kv.first.back() != UNK) kv.second.state = ns++;
  auto state_of = [&](const int* g, int n) -> int {   // the longest suffix of g (at most N - 1 words) that is a state
    for (int m = std::min(n, N - 1); m >= 1; --m) {
      const auto it = grams[m].find(Gram(g + n - m, g + n));
      if (it != grams[m].end() && it->second.state >= 0) return it->second.state;
    }
    return 0;
  };
  lm->bo_w.assign(ns, 0.f);
  lm->bo_next.assign(ns, 0);
  for (int n = 1; n < N; ++n)
    for (const auto& kv : grams[n])
      if (kv.second.state >= 0) {
        lm->bo_w[kv.second.state] = kv.second.bo;
        lm->bo_next[kv.second.state] = state_of(kv.first.data() + 1, n - 1);
      }
  const auto bos = grams[1].find(Gram{BOS});
  lm->start = bos != grams[1].end() ? bos->second.state : 0;   // (-1 when N == 1: fixed below)
  if (lm->start < 0) lm->start = 0;

  // ---- arcs, sorted by (state, class); state 0 first with its K - 1
  std::vector<std::tuple<int, int, float, int>> arcs;
  for (int c = 1; c < K; ++c) {
    const auto it = grams[1].find(Gram{c});
    const int g1[1] = {c};
    arcs.emplace_back(0, c, it != grams[1].end() ? it->second.w : unk->second.w, state_of(g1, 1));
  }
  for (int n = 2; n <= N; ++n)
    for (const auto& kv : grams[n]) {
      const int c = kv.first.back();
      if (c < 1 || c >= K) continue;   // predicts <s> (ignored), </s> (the state's final weight) or <unk> (never asked for)
      const int from = grams[n - 1].find(Gram(kv.first.begin(), kv.first.end() - 1))->second.state;
      if (from < 0) continue;          // a context that ends in </s> or <unk>: no hypothesis reaches it
      arcs.emplace_back(from, c, kv.second.w, state_of(kv.first.data(), n));
    }
  std::sort(arcs.begin(), arcs.end(), [](const auto& a, const auto& b) { return std::get<0>(a) != std::get<0>(b) ? std::get<0>(a) < std::get<0>(b) : std::get<1>(a) < std::get<1>(b); });
  if (arcs.size() >= ((size_t)1 << 31)) throw Error(EESEN_ERR_INVALID, std::string(arpa) + ": states and arcs must stay below 2^31");
  lm->arc_off.assign(ns + 1, 0);
  for (const auto& a : arcs) {
    lm->arc_off[std::get<0>(a) + 1]++;
    lm->arc_cls.push_back(std::get<1>(a));
    lm->arc_w.push_back(std::get<2>(a));
    lm->arc_next.push_back(std::get<3>(a));
  }
  for (int s = 0; s < ns; ++s) lm->arc_off[s + 1] += lm->arc_off[s];

  // ---- final weights: ln P(</s> | state), the backoff walk done here
  lm->has_eos = grams[1].count(Gram{EOS}) != 0;
  lm->fin.assign(ns, 0.f);
  lm->fin_abs.assign(ns, 0.0);
  if (lm->has_eos) {
    std::vector<float> eos_w(ns, 0.f);
    std::vector<char> eos_has(ns, 0);
    for (int n = 1; n <= N; ++n)
      for (const auto& kv : grams[n]) {
        if (kv.first.back() != EOS) continue;
        const int from = n == 1 ? 0 : grams[n - 1].find(Gram(kv.first.begin(), kv.first.end() - 1))->second.state;
        if (from >= 0) { eos_w[from] = kv.second.w; eos_has[from] = 1; }
      }
    for (int s = 0; s < ns; ++s) {
      double acc = 0, abs = 0;
      int h = s;
      while (!eos_has[h]) { acc += lm->bo_w[h]; abs += std::fabs((double)lm->bo_w[h]); h = lm->bo_next[h]; }   // (state 0 has it)
      lm->fin[s] = (float)(acc + eos_w[h]);
      lm->fin_abs[s] = abs + std::fabs((double)eos_w[h]);
    }
  }
}

// the arc of `state` for class c, or -1: state 0 is an index, every other state's sorted list is bisected
int TokenLm::find_arc(int state, int c) const {
  if (state == 0) return c - 1;
  const int* lo = arc_cls.data() + arc_off[state];
  const int* hi = arc_cls.data() + arc_off[state + 1];
  const int* it = std::lower_bound(lo, hi, c);
  return it != hi && *it == c ? (int)(it - arc_cls.data()) : -1;
}

void TokenLm::step(int state, int c, float* w, int* next) const {
  EESEN_REQUIRE(state >= 0 && state < states(), EESEN_ERR_INVALID, "LM state out of range");
  EESEN_REQUIRE(c >= 1 && c < K, EESEN_ERR_INVALID, "class id outside [1, K)");
  float acc = 0.f;
  int at;
  while ((at = find_arc(state, c)) < 0) {
    acc += bo_w[state];
    state = bo_next[state];
  }
  *w = acc + arc_w[at];
  *next = arc_next[at];
}

double TokenLm::score(const int* labels, int n, bool eos, double* abs_sum) const {
  EESEN_REQUIRE(!eos || has_eos, EESEN_ERR_INVALID, "use_eos on an LM whose file has no </s>");
  double sum = 0, abs = 0;
  int state = start;
  for (int i = 0; i < n; ++i) {
    const int c = labels[i];
    EESEN_REQUIRE(c >= 1 && c < K, EESEN_ERR_INVALID, "label outside [1, K)");
    int at;
    while ((at = find_arc(state, c)) < 0) {
      sum += bo_w[state];
      abs += std::fabs((double)bo_w[state]);
      state = bo_next[state];
    }
    sum += arc_w[at];
    abs += std::fabs((double)arc_w[at]);
    state = arc_next[at];
  }
  if (eos) { sum += fin[state]; abs += fin_abs[state]; }
  if (abs_sum) *abs_sum = abs;
  return sum;
}

}  // namespace eesen
