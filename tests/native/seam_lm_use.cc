// A host written against the C++ seam (include/eesen_hip_net.h) building an eesen::TokenLm and calling the eesen::Ctc::DecodeParallel
// overload that takes it: compiled, syntax only, by tests/test_ctc_lm_seam_compiles.py with the flags of the `seam` target of
// oracle/ref_build/Makefile.
#include "eesen_hip_net.h"

double decode(eesen::Ctc& ctc, const eesen::CuMatrix<eesen::BaseFloat>& net_out, const std::vector<eesen::int32>& frame_num_utt) {
  eesen::TokenLm lm("lm.arpa", "units.txt", net_out.NumCols());
  eesen::TokenLm ids("ids.arpa", "", net_out.NumCols());
  std::vector<std::vector<std::vector<eesen::int32> > > hyps;
  std::vector<std::vector<eesen::BaseFloat> > scores, lm_scores;
  ctc.DecodeParallel(frame_num_utt, net_out, lm, 0.8f, 0.5f, lm.HasEos(), &hyps, &scores);
  ctc.DecodeParallel(frame_num_utt, net_out, ids, 1.0f, 0.0f, false, &hyps, &scores, &lm_scores, 8, 10, 3, true);
  ctc.DecodeParallel(frame_num_utt, net_out, &hyps, &scores);          // the plain call is still there
  eesen::int32 next = 0;
  const eesen::BaseFloat w = lm.Step(lm.Start(), 1, &next);
  return w + lm.Final(next) + lm.Score(hyps[0][0], true) + lm.Order() + lm.NumStates() + lm.NumArcs();
}
