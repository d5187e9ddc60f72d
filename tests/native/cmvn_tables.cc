// Test harness (CPU only) for what compute-cmvn-stats adds to eesen_amd/csrc/tools/kaldi_tables.h and asks of feat_pipeline.h:
//   cmvn_tables weights <rspecifier>            `key n first last` per float vector
//   cmvn_tables spk2utt <rspecifier>            `spk utt utt ...` per speaker, in file order
//   cmvn_tables dm <rspecifier> <wspecifier>    copies a double-matrix table through read_matrix64 and DoubleMatrixWriter
//   cmvn_tables pipe <rspecifier>...            per feature rspecifier `source|stages|head` (the tap goes on boundary `stages`) or NONE
// Exit code 3 + the message on stderr when something throws.
#include <cstdio>
#include <cstring>
#include "../../eesen_amd/csrc/tools/feat_pipeline.h"
int main(int argc, char** argv) {
  if (argc < 3) return 1;
  try {
    if (!std::strcmp(argv[1], "weights")) {
      for (const auto& kv : ktab::read_float_vectors(argv[2]))
        std::printf("%s %zu %.9g %.9g\n", kv.first.c_str(), kv.second.size(), kv.second.empty() ? 0.0 : kv.second.front(), kv.second.empty() ? 0.0 : kv.second.back());
    } else if (!std::strcmp(argv[1], "spk2utt")) {
      for (const auto& kv : ktab::read_token_lists(argv[2])) {
        std::printf("%s", kv.first.c_str());
        for (const auto& u : kv.second) std::printf(" %s", u.c_str());
        std::printf("\n");
      }
    } else if (!std::strcmp(argv[1], "dm") && argc == 4) {
      std::vector<std::pair<std::string, ktab::Mat64>> items;
      ktab::read_whole_table<ktab::Mat64>(argv[2], ktab::read_matrix64, &items);
      ktab::DoubleMatrixWriter w(argv[3]);
      for (const auto& kv : items) w.Write(kv.first, kv.second.v.data(), kv.second.rows, kv.second.cols);
    } else if (!std::strcmp(argv[1], "pipe")) {
      for (int i = 2; i < argc; ++i) {
        ktab::Pipeline p;
        if (!ktab::parse_feature_pipeline(argv[i], &p)) { std::printf("NONE\n"); continue; }
        std::printf("%s|%zu|%s\n", p.source.c_str(), p.stages.size(), p.has_pitch ? "fbank+pitch" : p.has_fbank ? "fbank" : "table");
      }
    } else {
      return 1;
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;
  }
  return 0;
}
