// A host written against the C++ seam (include/eesen_hip_net.h) building an eesen::Lexicon and a word LM over its table and calling the
// eesen::Ctc::DecodeParallel overload that takes them: compiled, syntax only, by tests/test_ctc_lex_seam_compiles.py with the flags of
// the `seam` target of oracle/ref_build/Makefile.
#include "eesen_hip_net.h"

double decode(eesen::Ctc& ctc, const eesen::CuMatrix<eesen::BaseFloat>& net_out, const std::vector<eesen::int32>& frame_num_utt) {
  eesen::Lexicon lex("lexicon.txt", "units.txt", net_out.NumCols(), 1);
  eesen::Lexicon ids("lexicon_numbers.txt", "", net_out.NumCols(), 1);
  lex.WriteWords("words.txt");
  eesen::TokenLm lm("words.arpa", "words.txt", lex.NumWords() + 1);
  std::vector<std::vector<std::vector<eesen::int32> > > hyps, words;
  std::vector<std::vector<eesen::BaseFloat> > scores, lm_scores;
  ctc.DecodeParallel(frame_num_utt, net_out, lex, &lm, 0.8f, 0.5f, lm.HasEos(), &hyps, &words, &scores);
  ctc.DecodeParallel(frame_num_utt, net_out, ids, NULL, 1.0f, -0.5f, false, &hyps, &words, &scores, &lm_scores, 8, 10, 3, true);
  ctc.DecodeParallel(frame_num_utt, net_out, lm, 0.8f, 0.5f, false, &hyps, &scores);   // the token-LM call and the plain call are still there
  ctc.DecodeParallel(frame_num_utt, net_out, &hyps, &scores);
  std::vector<eesen::int32> segmented;
  const bool in_language = lex.Words(hyps[0][0], &segmented);
  return lm.Score(words[0][0], true) + lex.Word(lex.Child(0, 2)) + lex.NumNodes() + lex.MaxWordLength() + (in_language ? segmented.size() : 0);
}
