// A host written against the C++ seam (include/eesen_hip_net.h) asking eesen::Ctc::DecodeStamps for the time stamps and confidences of
// what a plain and a lexicon DecodeParallel returned: compiled, syntax only, by tests/test_ctc_stamps_seam_compiles.py with the flags of
// the `seam` target of oracle/ref_build/Makefile.
#include "eesen_hip_net.h"

double stamps(eesen::Ctc& ctc, const eesen::CuMatrix<eesen::BaseFloat>& net_out, const std::vector<eesen::int32>& frame_num_utt) {
  std::vector<std::vector<std::vector<eesen::int32> > > hyps, words;
  std::vector<std::vector<eesen::BaseFloat> > scores;
  eesen::Ctc::Stamps st;
  ctc.DecodeParallel(frame_num_utt, net_out, &hyps, &scores, 16, 20, 4);
  ctc.DecodeStamps(frame_num_utt, net_out, hyps, &st);
  double sum = st.path_score[0][0] + st.label_end[0][0].size() + st.word_conf[0][0].size();
  eesen::Lexicon lex("lexicon.txt", "units.txt", net_out.NumCols());
  ctc.DecodeParallel(frame_num_utt, net_out, lex, NULL, 1.0f, 0.0f, false, &hyps, &words, &scores, NULL, 16, 20, 4, true);
  ctc.DecodeStamps(frame_num_utt, net_out, hyps, &st, true, 0.5);
  for (size_t j = 0; j < st.word_start[0][0].size(); ++j) sum += 0.03 * (st.word_end[0][0][j] - st.word_start[0][0][j]) * st.word_conf[0][0][j];
  return sum + st.label_start[0][0].size();
}
