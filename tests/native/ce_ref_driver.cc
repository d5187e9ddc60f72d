// ce_ref_driver.cc -- test infrastructure: runs the REFERENCE's own eesen::CE (src/net/ce-loss.cc, compiled where it lies, CPU
// mode) over a sequence of minibatches read from a file, for tests/test_ce_restatement_vs_reference.py.
//   in : int32 ncalls, report_step; per call int32 rows, K, S, then float32 y[rows*K], int32 target[rows], float32 mask[rows]
//   out: per call float32 diff[rows*K], float64 obj_, int32 correct_, int32 frames_ (the running totals after the call)
// The progress lines go to stderr through KALDI_LOG; Report() goes to stdout.
#include <cstdio>
#include <vector>

#include "base/kaldi-common.h"   // everything ce-loss.h includes, first: only the CE class itself is opened up below
#include "util/kaldi-holder.h"
#include "gpucompute/cuda-matrix.h"
#include "gpucompute/cuda-vector.h"
#include "gpucompute/cuda-array.h"
#define private public   // the running totals (ce-loss.h:57-71) have no accessor
#include "net/ce-loss.h"
#undef private

using namespace eesen;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int hdr[2];
  if (std::fread(hdr, 4, 2, in) != 2) return 2;
  CE ce;
  ce.SetReportStep(hdr[1]);
  for (int c = 0; c < hdr[0]; ++c) {
    int d[3];
    if (std::fread(d, 4, 3, in) != 3) return 2;
    const int rows = d[0], K = d[1], S = d[2];
    std::vector<float> y((size_t)rows * K), mask(rows);
    std::vector<int32> tgt(rows);
    if (std::fread(y.data(), 4, y.size(), in) != y.size() || std::fread(tgt.data(), 4, rows, in) != (size_t)rows ||
        std::fread(mask.data(), 4, rows, in) != (size_t)rows) return 2;
    Matrix<BaseFloat> yh(rows, K);
    for (int r = 0; r < rows; ++r)
      for (int k = 0; k < K; ++k) yh(r, k) = y[(size_t)r * K + k];
    Vector<BaseFloat> mh(rows);
    for (int r = 0; r < rows; ++r) mh(r) = mask[r];
    CuMatrix<BaseFloat> net_out(yh), diff;
    if (S > 0) ce.EvalParallel(net_out, tgt, &diff, mh, S);
    else ce.Eval(net_out, tgt, &diff);
    Matrix<BaseFloat> dh(rows, K);
    diff.CopyToMat(&dh);
    for (int r = 0; r < rows; ++r) std::fwrite(dh.RowData(r), 4, K, out);
    const double obj = ce.obj_;
    const int32 tot[2] = {ce.correct_, ce.frames_};
    std::fwrite(&obj, 8, 1, out);
    std::fwrite(tot, 4, 2, out);
  }
  std::printf("%s", ce.Report().c_str());
  std::fclose(out);
  return 0;
}
