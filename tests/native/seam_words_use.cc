// A host written against the C++ seam (include/eesen_hip_net.h) building an unspaced eesen::Lexicon (no space class: the phoneme
// systems) and calling the eesen::Ctc::DecodeParallel overloads that take it, with and without the word ends: compiled, syntax only,
// by tests/test_ctc_words_seam_compiles.py with the flags of the `seam` target of oracle/ref_build/Makefile.
#include "eesen_hip_net.h"

double decode(eesen::Ctc& ctc, const eesen::CuMatrix<eesen::BaseFloat>& net_out, const std::vector<eesen::int32>& frame_num_utt) {
  eesen::Lexicon lex("lexicon.txt", "units.txt", net_out.NumCols());
  eesen::Lexicon spaced("lexicon_char.txt", "units.txt", net_out.NumCols(), 1);
  lex.WriteWords("words.txt");
  eesen::TokenLm lm("words.arpa", "words.txt", lex.NumWords() + 1);
  std::vector<std::vector<std::vector<eesen::int32> > > hyps, words, ends;
  std::vector<std::vector<eesen::BaseFloat> > scores, lm_scores;
  ctc.DecodeParallel(frame_num_utt, net_out, lex, &lm, 0.8f, 0.5f, lm.HasEos(), &hyps, &words, &ends, &scores);
  ctc.DecodeParallel(frame_num_utt, net_out, lex, NULL, 1.0f, -0.5f, false, &hyps, &words, &ends, &scores, &lm_scores, 8, 10, 3, true);
  ctc.DecodeParallel(frame_num_utt, net_out, lex, &lm, 0.8f, 0.5f, false, &hyps, &words, &scores);          // the overload without the ends dispatches too
  ctc.DecodeParallel(frame_num_utt, net_out, spaced, NULL, 1.0f, 0.0f, false, &hyps, &words, &ends, &scores);   // a spaced lexicon's ends: in front of every space
  const std::vector<eesen::int32> homophones = lex.NodeWords(lex.Child(0, 2));
  return lm.Score(words[0][0], true) + ends[0][0].size() + homophones.size() + lex.MaxHomophones() + (lex.Unspaced() ? 1 : 0) + spaced.SpaceClass();
}
