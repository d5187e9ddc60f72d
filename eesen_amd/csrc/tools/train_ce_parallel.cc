// train_ce_parallel.cc -- the reference's frame-level cross-entropy trainer (src/netbin/train-ce-parallel.cc) over the C-ABI of
// include/eesen_hip.h.
//
// Host C++ only: no HIP headers, no torch, no Python.  Same options, positional arguments, stderr protocol and exit codes as
// the reference binary, plus what the native CTC trainer registers for one job (--opt-algorithm, --adagrad-epsilon,
// --rms-prop-rho, --device).  The loop is the reference's (:108-170): greedy groups whose limit test comes AFTER an utterance
// is added (:132-136, so a group may exceed --frame-limit), then Propagate / CE / Backpropagate on the HIP path; minibatch
// padding + interleave + upload run on the device feeder's stream under the previous step (eesen_feeder_*), and the targets
// travel as int32 (eesen_ce_eval_parallel) instead of a dense one-hot matrix.
// Where the reference's behaviour is undefined this tool refuses instead ("CE"):
//   * a target vector whose length differs from its feature matrix is a WARNING; the utterance is skipped and counted under
//     "other errors" (the reference reads past the vector, :149);
//   * a final group left empty -- every remaining utterance lacked targets -- is not propagated (the reference runs a 0-row
//     minibatch through the Net).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/eesen_hip.h"
#include "../../../include/eesen_hip_info.h"
#include "kaldi_tables.h"
#include "parse_options.h"

namespace {
using namespace ktab;

void ck(int rc) {  // KALDI_ERR: message + std::runtime_error (src/base/kaldi-error.cc:168-182)
  if (rc != EESEN_OK) throw std::runtime_error(eesen_last_error());
}
void log_line(const char* level, const std::string& msg, const char* where = "main():eesen_amd/csrc/tools/train_ce_parallel.cc") {
  std::cerr << level << " (train-ce-parallel:" << where << ") " << msg << std::endl;
}
std::string fmt_g(double v) {  // what operator<< prints for a double by default
  std::ostringstream o;
  o << v;
  return o.str();
}

struct Options {  // train-ce-parallel.cc:40-61, NetTrainOptions train-opts.h:29-62
  float learn_rate = 0.008f, momentum = 0.f, adagrad_epsilon = 1e-6f, rms_prop_rho = 0.9f;
  bool binary = true, cross_validate = false;
  int num_sequence = 5, report_step = 100, verbose = 0, device = -1;
  double frame_limit = 100000;
  std::string use_gpu = "yes", opt_algorithm = "SGD";
  std::vector<std::string> args;
};
const char* kUsage =   // train-ce-parallel.cc:32-38
    "Perform one iteration of Cross-entropy (CE) training by SGD.\n"
    "The updates are done per-utternace and by processing multiple utterances in parallel.\n"
    "\n"
    "Usage: train-ce-parallel [options] <feature-rspecifier> <labels-rspecifier> <model-in> [<model-out>]\n"
    "e.g.: \n"
    "train-ce-parallel scp:feature.scp ark:labels.ark nnet.init nnet.iter1\n";

Options parse_options(int argc, char** argv, eesen_tools::ParseOptions* po) {
  Options o;
  po->Register("learn-rate", &o.learn_rate, "Learning rate");
  po->Register("momentum", &o.momentum, "Momentum");
  po->Register("adagrad-epsilon", &o.adagrad_epsilon, "Epsilon for numerical stability for all adaptive optimizers (Adagrad, RMSProp)");
  po->Register("rms-prop-rho", &o.rms_prop_rho, "Rho parameter for RMSProp");
  po->Register("binary", &o.binary, "Write model  in binary mode");
  po->Register("cross-validate", &o.cross_validate, "Perform cross-validation (no backpropagation)");
  po->Register("num-sequence", &o.num_sequence, "Number of sequences processed in parallel");
  po->Register("frame-limit", &o.frame_limit, "Max number of frames to be processed");
  po->Register("report-step", &o.report_step, "Step (number of sequences) for status reporting");
  po->Register("use-gpu", &o.use_gpu, "yes|no|optional, only has effect if compiled with CUDA");
  po->Register("opt-algorithm", &o.opt_algorithm, "Optimization algorithm (SGD|Adagrad|RMSProp)");
  po->Register("device", &o.device, "GPU index (default: $LOCAL_RANK, else 0)");
  po->Read(argc, argv);
  o.verbose = po->Verbose();
  for (int i = 1; i <= po->NumArgs(); ++i) o.args.push_back(po->GetArg(i));
  return o;
}

struct Minibatch {
  std::vector<Mat> mats;
  std::vector<std::vector<int32_t>> targets;
  std::vector<int> frames;
  int T = 0;
};

}  // namespace

int main(int argc, char** argv) {
  try {
    eesen_tools::ParseOptions po(kUsage);
    const Options o = parse_options(argc, argv, &po);
    if ((int)o.args.size() != 4 - (o.cross_validate ? 1 : 0)) {  // :64-67
      po.PrintUsage();
      return 1;
    }
    const std::string feature_rspecifier = o.args[0], targets_rspecifier = o.args[1], model_filename = o.args[2];
    const std::string target_model_filename = o.cross_validate ? "" : o.args[3];
    const int device = o.device >= 0 ? o.device : (getenv("LOCAL_RANK") ? atoi(getenv("LOCAL_RANK")) : 0);

    eesen_net_t* net = nullptr;
    eesen_ce_t* ce = nullptr;
    eesen_feeder_t* feeder = nullptr;
    ck(eesen_net_create(device, nullptr, &net));
    ck(eesen_net_read(net, model_filename.c_str()));                                   // :88
    ck(eesen_net_set_train_options(net, o.learn_rate, o.momentum));                    // :89
    ck(eesen_net_set_adaptive_options(net, o.adagrad_epsilon, o.rms_prop_rho));
    ck(eesen_net_set_update_algorithm(net, o.opt_algorithm.c_str()));
    ck(eesen_ce_create(device, nullptr, &ce));
    ck(eesen_ce_set_report_step(ce, o.report_step));                                   // :99
    ck(eesen_ce_set_guard(ce, net));   // a minibatch computed from a timed-out forward pass never reaches the statistics
    ck(eesen_feeder_create(device, nullptr, 2, &feeder));
    int feat_dim = 0, K = 0;
    ck(eesen_net_input_dim(net, &feat_dim));
    ck(eesen_net_output_dim(net, &K));

    FeatureReader feature_reader(feature_rspecifier);                                  // :94-95
    const std::map<std::string, std::vector<int32_t>> targets_reader = read_targets(targets_rspecifier);
    log_line("LOG", std::string(o.cross_validate ? "CROSS-VALIDATION" : "TRAINING") + " STARTED");   // :103
    const auto t0 = std::chrono::steady_clock::now();
    long num_done = 0, num_no_tgt_mat = 0, num_other_error = 0;
    double total_frames = 0;

    // the inner loop of :114-137: add utterances until num_sequence of them or more than frame_limit padded frames
    auto next_group = [&](Minibatch* mb) -> bool {
      mb->mats.clear(); mb->targets.clear(); mb->frames.clear(); mb->T = 0;
      int max_frame_num = 0;
      for (; !feature_reader.Done(); feature_reader.Next()) {
        const std::string utt = feature_reader.Key();
        auto tg = targets_reader.find(utt);
        if (tg == targets_reader.end()) {                                               // :117-122
          log_line("WARNING", utt + ", missing targets");
          ++num_no_tgt_mat;
          continue;
        }
        Mat& mat = feature_reader.Value();
        if ((long)tg->second.size() != mat.rows) {   // undefined behaviour in the reference (:149 reads labels_utt[s][r]): refused
          log_line("WARNING", utt + ", length mismatch of targets " + std::to_string(tg->second.size()) + " and features " + std::to_string(mat.rows));
          ++num_other_error;
          continue;
        }
        if (mat.cols != feat_dim) throw std::runtime_error("feature dimension " + std::to_string(mat.cols) + " does not match the net's InputDim " + std::to_string(feat_dim));
        max_frame_num = std::max(max_frame_num, mat.rows);                              // :127
        mb->frames.push_back(mat.rows);
        mb->targets.push_back(tg->second);
        mb->mats.push_back(std::move(mat));
        if ((int)mb->mats.size() == o.num_sequence || (double)mb->mats.size() * max_frame_num > o.frame_limit) {   // :132-136
          feature_reader.Next();
          break;
        }
      }
      mb->T = max_frame_num;
      return !mb->mats.empty();
    };
    auto stage = [&](const Minibatch& mb) -> int {  // padding + interleave + upload on the feeder's stream (replaces :139-151)
      std::vector<const float*> ptr(mb.mats.size());
      for (size_t s = 0; s < mb.mats.size(); ++s) ptr[s] = mb.mats[s].v.data();
      int slot = -1;
      ck(eesen_feeder_submit(feeder, ptr.data(), mb.frames.data(), nullptr, (int)mb.mats.size(), feat_dim, &slot));
      return slot;
    };
    char line[4096];
    auto print_progress = [&](int wait) {   // the KALDI_LOG of CE::EvalParallel (ce-loss.cc:153-167)
      for (;;) {
        ck(eesen_ce_progress(ce, wait, line, (int)sizeof(line)));
        if (!line[0]) break;
        log_line("LOG", line, "EvalParallel():eesen_amd/csrc/ce_host.cpp");
      }
    };

    Minibatch cur, nxt;
    bool have = next_group(&cur);   // an empty group: every remaining utterance lacked targets -- nothing to propagate
    int slot = have ? stage(cur) : -1;
    float* diff = nullptr;
    long diff_cap = 0;
    std::vector<int> target_host;
    while (have) {
      const int S = (int)cur.mats.size();
      float* feats = nullptr;
      int T = 0, S2 = 0, ld = 0;
      ck(eesen_feeder_acquire(feeder, slot, &feats, &T, &S2, &ld));
      ck(eesen_net_set_seq_lengths(net, cur.frames.data(), S));                        // :154
      const float* net_out = nullptr;
      int out_cols = 0, out_ld = 0;
      ck(eesen_net_propagate(net, feats, T * S, ld, /*in_is_device*/ 1, &net_out, &out_cols, &out_ld));   // :157
      ck(eesen_feeder_release(feeder, slot));
      target_host.assign((size_t)T * S, 0);                                             // :143-151
      for (int s = 0; s < S; ++s)
        for (int r = 0; r < cur.frames[s]; ++r) target_host[(size_t)r * S + s] = cur.targets[s][r];
      if ((long)T * S * out_ld > diff_cap) {   // (grows by half: the list is sorted by length, T rises from minibatch to minibatch)
        if (diff) { ck(eesen_net_synchronize(net)); ck(eesen_dev_free(device, diff)); }
        diff_cap = std::max((long)T * S * out_ld, diff_cap + diff_cap / 2);
        ck(eesen_dev_alloc(device, diff_cap * 4, reinterpret_cast<void**>(&diff)));
      }
      // does not wait for the device: the sums join the totals when they have arrived (the reference's call returns nothing)
      ck(eesen_ce_eval_parallel(ce, cur.frames.data(), S, net_out, T * S, out_cols, out_ld, target_host.data(), diff, out_ld, nullptr));  // :158
      if (!o.cross_validate) {                                                          // :161-163
        ck(eesen_net_backpropagate(net, diff, out_ld, nullptr, 0));
        ck(eesen_net_update(net));
      }
      print_progress(0);
      num_done += S;                                                                    // :165-166
      total_frames += (double)T * S;
      have = next_group(&nxt);                     // next batch: read and staged while the GPU runs this one's backward pass
      slot = have ? stage(nxt) : -1;
      std::swap(cur, nxt);
    }
    ck(eesen_net_synchronize(net));
    print_progress(1);
    if (!o.cross_validate) log_line("LOG", eesen_hip::NetInfo(net, 1, o.opt_algorithm != "SGD"));   // :172-174
    if (!o.cross_validate) ck(eesen_net_write(net, target_model_filename.c_str(), o.binary ? 1 : 0));   // :176-178
    const double el = std::max(1e-9, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    log_line("LOG", "Done " + std::to_string(num_done) + " files, " + std::to_string(num_no_tgt_mat) + " with no targets, " +
                        std::to_string(num_other_error) + " with other errors. [" + (o.cross_validate ? "CROSS-VALIDATION" : "TRAINING") + ", " +
                        fmt_g(el / 60) + " min, fps" + fmt_g(total_frames / el) + "]");              // :180-185
    long dropped = 0;
    ck(eesen_ce_dropped(ce, &dropped));
    if (dropped) log_line("WARNING", std::to_string(dropped) + " minibatch(es) were computed from a timed-out forward pass and are not in the statistics");
    ck(eesen_ce_report(ce, line, (int)sizeof(line)));
    log_line("LOG", line);                                                              // :186
    if (diff) eesen_dev_free(device, diff);
    eesen_feeder_destroy(feeder);
    eesen_ce_destroy(ce);
    eesen_net_destroy(net);
    return 0;
  } catch (const std::exception& e) {  // :193-196
    std::cerr << e.what() << std::endl;
    return 255;
  }
}
