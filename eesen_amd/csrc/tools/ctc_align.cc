// ctc_align.cc -- best-path CTC alignment of utterances against their transcripts, over the C-ABI of include/eesen_hip.h, host C++
// only.  The reference has no such binary: it aligns ONE utterance per invocation by compiling a TLG graph for it and running the
// WFST decoder over net-output-extract's output (asr_egs/wsj/steps/align_ctc_single_utt.sh:67-85).  Here, per group of
// --num-sequence utterances: Net::Feedforward as net-output-extract does it -> optional ClassPrior::SubtractOnLogpost (the options of
// net-output-extract; align_ctc_single_utt.sh:80 aligns on prior-scaled log-likelihoods) -> eesen_ctc_align_parallel.  Written: one
// int32 vector per utterance, the class id of every frame -- the targets table train-ce-parallel reads.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <iostream>
#include <sstream>

#include "../../../include/eesen_hip.h"
#include "kaldi_tables.h"
#include "feat_pipeline.h"
#include "class_prior.h"
#include "parse_options.h"

namespace {
using namespace ktab;

void ck(int rc) {
  if (rc != EESEN_OK) throw std::runtime_error(eesen_last_error());
}
}  // namespace

int main(int argc, char** argv) {
  try {
    std::string class_frame_counts, positions_wspecifier;
    float prior_scale = 1.f;
    double prior_cutoff = 1e-10, blank_scale = 1.0, frame_limit = 1e5;
    int num_sequence = 1, device = 0;
    std::string use_gpu = "yes";
    eesen_tools::ParseOptions po(
        "Align utterances against their label sequences: the best (Viterbi) CTC path through the network's outputs.\n"
        "Writes the class id of every frame (blank = 0), the targets table of train-ce-parallel.\n"
        "\n"
        "Usage:  ctc-align [options] <model-in> <feature-rspecifier> <labels-rspecifier> <alignment-wspecifier>\n"
        "e.g.: \n"
        "ctc-align net ark:features.ark ark:labels.ark ark:ali.ark\n");
    po.Register("class-frame-counts", &class_frame_counts, "Vector with frame-counts of classes to compute log-priors; the alignment then runs on "
                                                           "log-posteriors minus the scaled log-priors");
    po.Register("prior-scale", &prior_scale, "Scaling factor to be applied on class-log-priors");
    po.Register("prior-cutoff", &prior_cutoff, "Classes with priors lower than cutoff will have 0 likelihood");
    po.Register("blank-scale", &blank_scale, "Scale probability of class 0 (blank) by this factor");
    po.Register("positions-wspecifier", &positions_wspecifier, "Also write the lattice position of every frame (position j of the labels interleaved "
                                                               "with blanks: label j/2 when j is odd, a blank otherwise)");
    po.Register("use-gpu", &use_gpu, "yes|no|optional (accepted for the recipes' command lines; this tool always runs on the GPU)");
    po.Register("num-sequence", &num_sequence, "Utterances forwarded and aligned together");
    po.Register("frame-limit", &frame_limit, "Max number of frames forwarded together");
    po.Register("device", &device, "GPU index");
    po.Read(argc, argv);
    std::vector<std::string> args;
    for (int i = 1; i <= po.NumArgs(); ++i) args.push_back(po.GetArg(i));
    if (args.size() != 4) {
      po.PrintUsage();
      return 1;
    }
    eesen_net_t* net = nullptr;
    eesen_feeder_t* feeder = nullptr;
    eesen_ctc_t* ctc = nullptr;
    ck(eesen_net_create(device, nullptr, &net));
    ck(eesen_net_read(net, args[0].c_str()));
    ck(eesen_net_set_train_mode(net, 0));
    ck(eesen_feeder_create(device, nullptr, 1, &feeder));
    ck(eesen_ctc_create(device, nullptr, &ctc));
    ck(eesen_ctc_set_guard(ctc, net));       // an alignment of a timed-out forward pass comes back as NaN, never as a table entry
    int D = 0, K = 0;
    ck(eesen_net_input_dim(net, &D));
    ck(eesen_net_output_dim(net, &K));
    std::vector<float> log_pri;
    if (!class_frame_counts.empty()) {
      log_pri = class_log_priors(class_frame_counts, prior_cutoff, blank_scale);
      if ((int)log_pri.size() != K)
        throw std::runtime_error("Dimensionality mismatch, class_frame_counts " + std::to_string(log_pri.size()) + " class_output_llk " + std::to_string(K));
    }
    // feature pipes (`apply-cmvn ... | splice-feats ... |`) as net-output-extract recognises them: the raw table is read here and the
    // filters run on the device (feat_pipeline.h)
    Pipeline pipe;
    const bool piped = !getenv("EESEN_HOST_FEATURE_PIPES") && parse_feature_pipeline(args[1], &pipe);
    std::unique_ptr<CmvnTable> cmvn_table;
    if (piped) {
      ck(pipe.configure(feeder));
      if (!pipe.cmvn.empty()) cmvn_table.reset(new CmvnTable(pipe.cmvn, pipe.utt2spk, pipe.norm_vars));
    }
    const std::map<std::string, std::vector<int32_t>> labels = read_targets(args[2]);
    FeatureReader reader(piped ? pipe.source : args[1], piped ? pipe.wave_mode() : nullptr);
    IntVectorWriter writer(args[3]);
    std::unique_ptr<IntVectorWriter> pos_writer;
    if (!positions_wspecifier.empty()) pos_writer.reset(new IntVectorWriter(positions_wspecifier));
    long num_done = 0, num_no_labels = 0, num_infeasible = 0;
    double tot_t = 0, tot_score = 0;
    std::vector<std::pair<std::string, Mat>> group;
    std::vector<int> out_frames;            // per utterance of the group: frames behind the pipeline
    std::vector<const float*> cmvn;
    std::vector<int> ali, pos, lab_ids, lab_off;
    std::vector<float> score;
    auto flush = [&]() {
      const int S = (int)group.size();
      std::vector<const float*> ptr(S);
      std::vector<int> frames(out_frames), raw_frames(S);
      lab_ids.clear(); lab_off.assign(1, 0);
      for (int s = 0; s < S; ++s) {
        ptr[s] = group[s].second.v.data(); raw_frames[s] = group[s].second.rows;
        const std::vector<int32_t>& l = labels.at(group[s].first);
        lab_ids.insert(lab_ids.end(), l.begin(), l.end());
        lab_off.push_back((int)lab_ids.size());
      }
      int slot = 0, T = 0, S2 = 0, ld = 0;
      float* feats = nullptr;
      if (piped) ck(eesen_feeder_submit_raw(feeder, ptr.data(), raw_frames.data(), nullptr, cmvn_table ? cmvn.data() : nullptr, S, group[0].second.cols, &slot));
      else ck(eesen_feeder_submit(feeder, ptr.data(), frames.data(), nullptr, S, D, &slot));
      ck(eesen_feeder_acquire(feeder, slot, &feats, &T, &S2, &ld));
      ck(eesen_net_set_seq_lengths(net, frames.data(), S));
      const float* out = nullptr;
      int oc = 0, old = 0;
      ck(eesen_net_propagate(net, feats, T * S, ld, 1, &out, &oc, &old));
      ck(eesen_feeder_release(feeder, slot));
      if (!log_pri.empty())
        ck(eesen_op_log_sub_prior(device, nullptr, const_cast<float*>(out), T * S, K, old, 1, log_pri.data(), prior_scale));
      ali.resize((size_t)T * S); pos.resize((size_t)T * S); score.resize(S);
      ck(eesen_ctc_align_parallel(ctc, frames.data(), S, out, T * S, K, old, log_pri.empty() ? 0 : 1, lab_ids.data(), lab_off.data(), ali.data(),
                                  pos.data(), score.data()));
      for (int s = 0; s < S; ++s) {  // rows t*S + s
        if (std::isnan(score[s])) throw std::runtime_error("the forward pass of " + group[s].first + " timed out on the device: no alignment");
        if (!(score[s] > -1e29f)) {
          std::cerr << "WARNING (ctc-align:main()) " << group[s].first << ", no feasible alignment of " << lab_off[s + 1] - lab_off[s] << " labels on "
                    << frames[s] << " frames, producing no output for this utterance" << std::endl;
          ++num_infeasible;
          continue;
        }
        writer.Write(group[s].first, ali.data() + s, frames[s], S);
        if (pos_writer) pos_writer->Write(group[s].first, pos.data() + s, frames[s], S);
        ++num_done;
        tot_t += frames[s];
        tot_score += score[s];
      }
      group.clear(); out_frames.clear(); cmvn.clear();
    };
    int max_len = 0;
    for (; !reader.Done(); reader.Next()) {
      Mat& m = reader.Value();
      int rows = m.rows, cols = m.cols;
      const float* cm = nullptr;
      const std::string& utt = reader.Key();
      if (piped) {  // what the filters would have dropped (apply-cmvn.cc:87-92, add-deltas.cc:55-58, subsample-feats.cc:87-92)
        if (cmvn_table) {
          const std::vector<float>* n = cmvn_table->lookup(utt);
          if (!n) { std::cerr << "WARNING (ctc-align:main()) No normalization statistics available for key " << utt << ", producing no output for this utterance" << std::endl; continue; }
          if (CmvnTable::dim(*n) != pipe.cmvn_dim(m.cols))
            throw std::runtime_error("Dim mismatch in ApplyCmvn: cmvn 2x" + std::to_string(CmvnTable::dim(*n) + 1) + ", feats " + std::to_string(m.rows) + "x" + std::to_string(m.cols));
          cm = n->data();
        }
        if (m.rows == 0) { std::cerr << "WARNING (ctc-align:main()) Empty feature matrix for key " << utt << std::endl; continue; }
        ck(eesen_feeder_pipeline_shape(feeder, m.cols, m.rows, &cols, &rows));
        if (rows == 0) { std::cerr << "WARNING (ctc-align:main()) For utterance " << utt << ", output would have no rows, producing no output." << std::endl; continue; }
      }
      const auto lab = labels.find(utt);
      if (lab == labels.end() || lab->second.empty()) {
        std::cerr << "WARNING (ctc-align:main()) " << utt << ", missing labels" << std::endl;
        ++num_no_labels;
        continue;
      }
      if (cols != D) throw std::runtime_error("feature dimension " + std::to_string(cols) + " does not match the net's InputDim " + std::to_string(D));
      if (!group.empty() && ((int)group.size() == num_sequence || (double)std::max(max_len, rows) * (group.size() + 1) > frame_limit)) {
        flush();
        max_len = 0;
      }
      max_len = std::max(max_len, rows);
      out_frames.push_back(rows);
      cmvn.push_back(cm);
      group.emplace_back(utt, std::move(m));
    }
    if (!group.empty()) flush();
    std::cerr << "LOG (ctc-align:main()) Done " << num_done << " utterances, " << num_no_labels << " without labels, " << num_infeasible
              << " infeasible; average best-path log-score per frame " << (tot_t > 0 ? tot_score / tot_t : 0.0) << std::endl;
    eesen_ctc_destroy(ctc);
    eesen_feeder_destroy(feeder);
    eesen_net_destroy(net);
    return num_done ? 0 : 255;
  } catch (const std::exception& e) {
    std::cerr << "ERROR (ctc-align:main()) " << e.what() << std::endl;
    return 255;
  }
}
