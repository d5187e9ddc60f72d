// A host written against the C++ seam (include/eesen_hip_net.h) calling eesen::Ctc::AlignParallel: compiled, syntax only, by
// tests/test_ctc_align_seam_compiles.py with the flags of the `seam` target of oracle/ref_build/Makefile.
#include "eesen_hip_net.h"

void align(eesen::Ctc& ctc, const eesen::CuMatrix<eesen::BaseFloat>& net_out, const std::vector<eesen::int32>& frame_num_utt,
           std::vector<std::vector<eesen::int32> >& label) {
  std::vector<eesen::int32> ali, pos;
  std::vector<eesen::BaseFloat> score;
  ctc.AlignParallel(frame_num_utt, net_out, label, &ali, &pos, &score);
  ctc.AlignParallel(frame_num_utt, net_out, label, &ali, NULL, &score, true);
}
