// lex_lm_malformed.cc -- feeds malformed (and a few well-formed) lexicon and ARPA files straight through eesen::Lexicon::from_file
// (csrc/lex.cpp) and eesen::TokenLm::from_arpa (csrc/lm.cpp).  Host code only: tests/test_lex_compile.py builds it together with the
// two sources under -fsanitize=address,undefined and runs it.  Every malformed file must end in an eesen::Error whose message holds
// the expected words; anything else -- no error, another exception, a sanitizer report -- fails the run.
//   usage: lex_lm_malformed <scratch directory>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../eesen_amd/csrc/common.h"
#include "../../eesen_amd/csrc/lex.h"
#include "../../eesen_amd/csrc/lm.h"

namespace {

int failures = 0;
std::string dir;

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

void lex(const std::string& text, const char* units, int K, int space) {
  eesen::Lexicon l;
  l.from_file(put("lex.txt", text).c_str(), units, K, space);
  // walk what was built: every edge, and a segmentation that leaves the language at every position
  std::vector<int> lab, out(64);
  for (int v = 0; v < l.nodes(); ++v)
    for (int c = 0; c <= K; ++c)
      if (c >= 1 && c < K) (void)l.child(v, c);
  for (int c = 1; c < K; ++c) {
    lab.assign(9, c);
    int n = 0;
    (void)l.words(lab.data(), (int)lab.size(), out.data(), &n);
  }
  l.write_words((dir + "/words.txt").c_str());
}

void arpa(const std::string& text, const char* units, int K, bool skip_oov) {
  eesen::TokenLm m;
  m.from_arpa(put("lm.arpa", text).c_str(), units, K, skip_oov);
  for (int s = 0; s < m.states(); ++s)
    for (int c = 1; c < K; ++c) {
      float w;
      int next;
      m.step(s, c, &w, &next);
    }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s <scratch directory>\n", argv[0]); return 2; }
  dir = argv[1];
  const std::string units = put("units.txt", "<SPACE> 1\na 2\nb 3\n");
  const char* u = units.c_str();

  accept("lexicon with a prefix word, two spellings and a repeated line", [&] { lex("a a\nab a b\nba b a\nba b b a\nab a b\n\n", u, 4, 1); });
  accept("lexicon of decimal ids", [&] { lex("x 2\ny 2 3\n", nullptr, 4, 1); });
  refuse("unknown unit", "not in the units table", [&] { lex("a a\nc a c\n", u, 4, 1); });
  refuse("non-decimal unit without a table", "no decimal class id", [&] { lex("a 2\nb x\n", nullptr, 4, 1); });
  refuse("the space inside a spelling", "space class", [&] { lex("a a <SPACE> a\n", u, 4, 1); });
  refuse("a unit outside [1, K)", "outside [1, K)", [&] { lex("a 2 4\n", nullptr, 4, 1); });
  refuse("the blank inside a spelling", "outside [1, K)", [&] { lex("a 0\n", nullptr, 4, 1); });
  refuse("a unit of twenty digits", "no decimal class id", [&] { lex("a 99999999999999999999\n", nullptr, 4, 1); });
  refuse("empty spelling", "empty spelling", [&] { lex("a a\nb\n", u, 4, 1); });
  refuse("one spelling for two words", "words a and b have the same spelling", [&] { lex("a a b\nb a b\n", u, 4, 1); });
  refuse("empty file", "holds no word", [&] { lex("", u, 4, 1); });
  refuse("blank lines only", "holds no word", [&] { lex("\n   \n\t\n", u, 4, 1); });
  refuse("a file that does not exist", "cannot open", [&] { eesen::Lexicon l; l.from_file((dir + "/none.txt").c_str(), u, 4, 1); });
  refuse("a units table that does not exist", "cannot open", [&] { lex("a a\n", (dir + "/none.txt").c_str(), 4, 1); });
  refuse("a space class outside [1, K)", "space class", [&] { lex("a 2\n", nullptr, 4, 4); });
  refuse("a line without a newline that ends in a bad unit", "not in the units table", [&] { lex("a a\nb q", u, 4, 1); });

  const std::string words = put("w.txt", "a 1\nab 2\nba 3\n");
  const char* w = words.c_str();
  const std::string head = "\\data\\\nngram 1=6\nngram 2=3\n\n\\1-grams:\n-99 <s> -0.3\n-1 </s>\n-0.5 a -0.2\n-0.6 ab -0.1\n-0.7 ba\n-0.9 zebra -0.4\n\n";
  const std::string oov = head + "\\2-grams:\n-0.2 a zebra\n-0.3 zebra ab\n-0.4 a ab\n\n\\end\\\n";
  accept("ARPA with out-of-vocabulary n-grams, skip_oov", [&] { arpa(oov, w, 4, true); });
  refuse("the same file without skip_oov", "zebra", [&] { arpa(oov, w, 4, false); });
  refuse("skip_oov: the section counts still have to agree", "the header says", [&] { arpa(head + "\\2-grams:\n-0.2 a zebra\n-0.4 a ab\n\n\\end\\\n", w, 4, true); });
  refuse("skip_oov: a word without a unigram and no <unk>", "has no unigram", [&] { arpa("\\data\\\nngram 1=2\n\n\\1-grams:\n-1 a\n-1 zebra\n\n\\end\\\n", w, 4, true); });
  refuse("no \\data\\ section", "no \\data\\", [&] { arpa("ngram 1=1\n", w, 4, true); });
  refuse("a non-numeric value", "not a finite number", [&] { arpa("\\data\\\nngram 1=1\n\n\\1-grams:\nx a\n", w, 4, true); });
  refuse("an n-gram line cut short", "needs a value", [&] { arpa("\\data\\\nngram 1=1\nngram 2=1\n\n\\1-grams:\n-1 a\n\\2-grams:\n-1 a\n", w, 4, true); });
  refuse("a prefix that is not listed", "prefix of this n-gram is not listed", [&] { arpa("\\data\\\nngram 1=3\nngram 2=1\n\n\\1-grams:\n-1 a\n-1 ab\n-1 <unk>\n\\2-grams:\n-1 ba a\n", w, 4, true); });
  refuse("a decimal class id outside [1, K) without a table", "no class id", [&] { arpa("\\data\\\nngram 1=1\n\n\\1-grams:\n-1 7\n", nullptr, 4, false); });

  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
