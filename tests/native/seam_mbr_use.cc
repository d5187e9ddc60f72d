// A host written against the C++ seam (include/eesen_hip_net.h) asking eesen::Ctc::EditDistanceParallel for distances among sequences of
// its own and eesen::Ctc::MbrNbest for the minimum Bayes risk order of what a plain and a lexicon DecodeParallel returned, alone and
// over RescoreNbest's totals: compiled, syntax only, by tests/test_mbr_seam_compiles.py with the flags of the `seam` target of
// oracle/ref_build/Makefile.
#include "eesen_hip_net.h"

double mbr(eesen::Ctc& ctc, const eesen::CuMatrix<eesen::BaseFloat>& net_out, const std::vector<eesen::int32>& frame_num_utt,
           const std::vector<std::vector<eesen::int32> >& refs) {
  std::vector<std::vector<std::vector<eesen::int32> > > hyps, words;
  std::vector<std::vector<eesen::BaseFloat> > scores;
  ctc.DecodeParallel(frame_num_utt, net_out, &hyps, &scores, 8, 20, 8);
  std::vector<std::vector<eesen::int32> > pair, ref_dist;
  ctc.EditDistanceParallel(hyps, &pair);
  ctc.EditDistanceParallel(hyps, &pair, &refs, &ref_dist);
  double sum = pair[0][1] + ref_dist[0][0];
  const eesen::int32 S = (eesen::int32)frame_num_utt.size();
  eesen::Ctc::Mbr m;
  ctc.MbrNbest(S, &m);
  sum += m.risk[0][m.order[0][0]] + m.posterior[0][0] + m.dist[0][1];
  eesen::Ctc::Rescored r;
  ctc.RescoreNbest(frame_num_utt, net_out, hyps, &r);
  ctc.MbrNbest(S, &m, 0, 0.5, &r.total, &refs);
  sum += m.ref_dist[0][m.order[0][0]] + hyps[0][m.order[0][0]].size();
  eesen::Lexicon lex("lexicon.txt", "units.txt", net_out.NumCols());
  ctc.DecodeParallel(frame_num_utt, net_out, lex, NULL, 1.0f, 0.0f, false, &hyps, &words, &scores, NULL, 16, 20, 4, true);
  ctc.MbrNbest(S, &m, 1);
  return sum + words[0][m.order[0][0]].size() + m.risk[0].size();
}
