// words_lex_malformed.cc -- feeds well-formed and malformed lexicon files straight through eesen::Lexicon::from_file_unspaced
// (csrc/lex.cpp: no boundary unit, several words per spelling) and walks the tables it built.  Host code only:
// tests/test_words_lex_compile.py builds it together with lex.cpp and lm.cpp under -fsanitize=address,undefined and runs it.  Every
// malformed file must end in an eesen::Error whose message holds the expected words; anything else -- no error, another exception, a
// sanitizer report -- fails the run.
//   usage: words_lex_malformed <scratch directory>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../eesen_amd/csrc/common.h"
#include "../../eesen_amd/csrc/lex.h"

namespace {

int failures = 0;
std::string dir;
volatile long sink;   // keeps the table reads alive

std::string put(const std::string& name, const std::string& text) {
  const std::string path = dir + "/" + name;
  std::ofstream(path, std::ios::binary) << text;
  return path;
}

template <typename F>
void refuse(const char* what, const std::string& words, F&& run) {
  try {
    run();
    std::printf("FAIL %s: accepted\n", what);
    ++failures;
  } catch (const eesen::Error& e) {
    const bool ok = std::string(e.what()).find(words) != std::string::npos && e.code == EESEN_ERR_INVALID;
    std::printf("%s %s: %s\n", ok ? "ok  " : "FAIL", what, e.what());
    failures += !ok;
  }
}

template <typename F>
void accept(const char* what, F&& run) {
  try {
    run();
    std::printf("ok   %s\n", what);
  } catch (const std::exception& e) {
    std::printf("FAIL %s: %s\n", what, e.what());
    ++failures;
  }
}

// compiles the text and reads every table entry the device copy would hold; returns H
int lex(const std::string& text, const char* units, int K) {
  eesen::Lexicon l;
  l.from_file_unspaced(put("lex.txt", text).c_str(), units, K);
  long sum = 0;
  for (int v = 0; v < l.nodes(); ++v) {
    for (int c = 1; c < K; ++c) sum += l.child(v, c);
    for (int i = 0; i < l.wcount[v]; ++i) sum += l.node_words[l.wfirst[v] + i];
    if (l.wcount[v] > l.max_homophones || (l.wcount[v] > 0) != (l.word[v] != 0)) { std::printf("FAIL node %d: its word list and its word disagree\n", v); ++failures; }
  }
  if ((size_t)(l.wfirst.back() + l.wcount.back()) != l.node_words.size()) { std::printf("FAIL the word lists do not tile node_words\n"); ++failures; }
  l.write_words((dir + "/words.txt").c_str());
  sink = sum;
  return l.max_homophones;
}

std::string homophones(int n) {
  std::string text = "other c\n";
  for (int i = 0; i < n; ++i) text += "h" + std::to_string(i) + " a b\n";
  return text;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s <scratch directory>\n", argv[0]); return 2; }
  dir = argv[1];
  const std::string units = put("units.txt", "a 1\nb 2\nc 3\n");
  const char* u = units.c_str();

  accept("a prefix word, homophones, two spellings and a repeated line", [&] {
    if (lex("a a\nab a b\nto b c\ntwo b c\nba b a\nba b b a\nab a b\ntoo b c\n\n", u, 4) != 3) throw std::runtime_error("H is not 3");
  });
  accept("decimal ids, K = 2", [&] { lex("x 1\nxx 1 1\n", nullptr, 2); });
  accept("fifteen words on one spelling, one of them twice", [&] {
    if (lex(homophones(15) + "h7 a b\n", u, 4) != 15) throw std::runtime_error("H is not 15");
  });
  refuse("the sixteenth word on one spelling", "15 words with the same spelling (the first of them: h0, line 2)", [&] { lex(homophones(16), u, 4); });
  refuse("unknown unit", "not in the units table", [&] { lex("a a\nc a q\n", u, 4); });
  refuse("non-decimal unit without a table", "no decimal class id", [&] { lex("a 2\nb x\n", nullptr, 4); });
  refuse("a unit outside [1, K)", "outside [1, K)", [&] { lex("a 2 4\n", nullptr, 4); });
  refuse("the blank inside a spelling", "outside [1, K)", [&] { lex("a 0\n", nullptr, 4); });
  refuse("a negative unit", "no decimal class id", [&] { lex("a -1\n", nullptr, 4); });
  refuse("a unit of twenty digits", "no decimal class id", [&] { lex("a 99999999999999999999\n", nullptr, 4); });
  refuse("empty spelling", "empty spelling", [&] { lex("a a\nb\n", u, 4); });
  refuse("empty file", "holds no word", [&] { lex("", u, 4); });
  refuse("blank lines only", "holds no word", [&] { lex("\n   \n\t\n", u, 4); });
  refuse("a file that does not exist", "cannot open", [&] { eesen::Lexicon l; l.from_file_unspaced((dir + "/none.txt").c_str(), u, 4); });
  refuse("a units table that does not exist", "cannot open", [&] { lex("a a\n", (dir + "/none.txt").c_str(), 4); });
  refuse("K = 1", "K >= 2", [&] { lex("a 1\n", nullptr, 1); });
  refuse("a line without a newline that ends in a bad unit", "not in the units table", [&] { lex("a a\nb q", u, 4); });
  refuse("segmenting a labelling", "ambiguous", [&] {
    eesen::Lexicon l;
    l.from_file_unspaced(put("lex.txt", "a a\n").c_str(), u, 4);
    int lab[1] = {1}, out[2], n = 0;
    (void)l.words(lab, 1, out, &n);
  });
  // the spaced kind beside it: unchanged, and without the unspaced tables
  accept("a lexicon with a space class", [&] {
    eesen::Lexicon l;
    l.from_file(put("lex.txt", "a 2\nab 2 3\n").c_str(), nullptr, 4, 1);
    if (l.unspaced || l.max_homophones != 0 || !l.node_words.empty() || !l.wfirst.empty()) throw std::runtime_error("the spaced kind grew homophone tables");
  });
  refuse("homophones in a lexicon with a space class", "have the same spelling", [&] {
    eesen::Lexicon l;
    l.from_file(put("lex.txt", "a 2 3\nb 2 3\n").c_str(), nullptr, 4, 1);
  });

  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
