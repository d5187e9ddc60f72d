// A host written against the C++ seam (include/eesen_hip_net.h) calling eesen::Ctc::DecodeParallel: compiled, syntax only, by
// tests/test_ctc_decode_seam_compiles.py with the flags of the `seam` target of oracle/ref_build/Makefile.
#include "eesen_hip_net.h"

void decode(eesen::Ctc& ctc, const eesen::CuMatrix<eesen::BaseFloat>& net_out, const std::vector<eesen::int32>& frame_num_utt) {
  std::vector<std::vector<std::vector<eesen::int32> > > hyps;
  std::vector<std::vector<eesen::BaseFloat> > scores;
  ctc.DecodeParallel(frame_num_utt, net_out, &hyps, &scores);
  ctc.DecodeParallel(frame_num_utt, net_out, &hyps, &scores, 8, 10, 3, true);
}
