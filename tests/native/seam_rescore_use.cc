// A host written against the C++ seam (include/eesen_hip_net.h) asking eesen::Ctc::ScoreParallel for the exact scores of labellings of
// its own and eesen::Ctc::RescoreNbest for a second pass over what a plain and a lexicon DecodeParallel returned: compiled, syntax only,
// by tests/test_ctc_rescore_seam_compiles.py with the flags of the `seam` target of oracle/ref_build/Makefile.
#include "eesen_hip_net.h"

double rescore(eesen::Ctc& ctc, const eesen::CuMatrix<eesen::BaseFloat>& net_out, const std::vector<eesen::int32>& frame_num_utt) {
  std::vector<std::vector<std::vector<eesen::int32> > > hyps, words;
  std::vector<std::vector<eesen::BaseFloat> > scores, exact;
  ctc.DecodeParallel(frame_num_utt, net_out, &hyps, &scores, 4, 20, 4);
  ctc.ScoreParallel(frame_num_utt, net_out, hyps, &exact);
  double sum = exact[0][0] - scores[0][0];
  eesen::Ctc::Rescored r;
  ctc.RescoreNbest(frame_num_utt, net_out, hyps, &r);
  sum += r.total[0][r.order[0][0]] + r.am_score[0][0] + r.lm_score[0][0];
  eesen::TokenLm second("second.arpa", "units.txt", net_out.NumCols());
  ctc.RescoreNbest(frame_num_utt, net_out, hyps, &r, &second, 0.8f, 0.5f, true);
  sum += hyps[0][r.order[0][0]].size();
  eesen::Lexicon lex("lexicon.txt", "units.txt", net_out.NumCols());
  ctc.DecodeParallel(frame_num_utt, net_out, lex, NULL, 1.0f, 0.0f, false, &hyps, &words, &scores, NULL, 16, 20, 4, true);
  ctc.RescoreNbest(frame_num_utt, net_out, hyps, &r, NULL, 1.0f, 0.3f, false, true);
  return sum + words[0][r.order[0][0]].size() + r.total[0].size();
}
