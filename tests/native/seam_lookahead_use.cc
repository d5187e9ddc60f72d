// A host written against the C++ seam (include/eesen_hip_net.h) asking eesen::Lexicon for the unigram look-ahead table of a word LM and
// decoding with eesen::Ctc::SetLmLookahead along both kinds of lexicon: compiled, syntax only, by tests/test_ctc_lookahead_seam_compiles.py
// with the flags of the `seam` target of oracle/ref_build/Makefile.
#include "eesen_hip_net.h"

double decode(eesen::Ctc& ctc, const eesen::CuMatrix<eesen::BaseFloat>& net_out, const std::vector<eesen::int32>& frame_num_utt) {
  eesen::Lexicon lex("lexicon.txt", "units.txt", net_out.NumCols());
  eesen::Lexicon spaced("lexicon_char.txt", "units.txt", net_out.NumCols(), 1);
  lex.WriteWords("words.txt");
  eesen::TokenLm lm("words.arpa", "words.txt", lex.NumWords() + 1);
  const std::vector<eesen::BaseFloat> la = lex.Lookahead(lm);
  std::vector<std::vector<std::vector<eesen::int32> > > hyps, words, ends;
  std::vector<std::vector<eesen::BaseFloat> > scores;
  ctc.SetLmLookahead(1);
  ctc.DecodeParallel(frame_num_utt, net_out, lex, &lm, 0.8f, 0.5f, lm.HasEos(), &hyps, &words, &ends, &scores);
  ctc.DecodeParallel(frame_num_utt, net_out, spaced, &lm, 0.8f, 0.5f, false, &hyps, &words, &scores);
  const eesen::int32 mode = ctc.LmLookahead();
  ctc.SetLmLookahead(0);
  return la[0] + la[lex.Child(0, 2)] + mode + scores[0][0] + spaced.Lookahead(lm).size();
}
