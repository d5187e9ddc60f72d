// process_kaldi_pitch_feats.cc -- process-kaldi-pitch-feats over the C-ABI: (NCCF, pitch) pairs to ASR features, on the device.
//
// Usage: process-kaldi-pitch-feats [options...] <feat-rspecifier> <feats-wspecifier>
// The reference's tool (src/featbin/process-kaldi-pitch-feats.cc) with the option names of ProcessPitchOptions::Register and its exit
// status (1 when nothing was done); matrices are batched by total frames and every batch is one launch (eesen_pitch_process,
// INTEGRATION.md "Pitch").  Deviations: the delta-pitch noise is a counter-based generator keyed by --noise-seed, the utterance's
// number in the table and the frame, so a run reproduces (--srand is accepted and unused; --delta-pitch-noise-stddev=0 is the
// path held to the reference); an empty input matrix is skipped with a warning.
#include <iostream>
#include <string>
#include <vector>

#include "../../../include/eesen_hip.h"
#include "kaldi_tables.h"
#include "parse_options.h"

using namespace ktab;

static void ck(int rc) {
  if (rc != EESEN_OK) throw std::runtime_error(eesen_last_error());
}

int main(int argc, char** argv) {
  try {
    eesen_pitch_opts_t o;
    eesen_pitch_opts_default(&o);
    bool add_pov_feature = true, add_normalized_log_pitch = true, add_delta_pitch = true, add_raw_log_pitch = false;
    int device = 0, noise_seed = 0, srand_seed = 0;
    eesen_tools::ParseOptions po(
        "Post-process Kaldi pitch features, consisting of pitch and NCCF, into\n"
        "features suitable for input to ASR system.  Default setup produces\n"
        "3-dimensional features consisting of (pov-feature, pitch-feature,\n"
        "delta-pitch-feature); select from (pov-feature, pitch-feature,\n"
        "delta-pitch-feature, raw-log-pitch), produced in that order, with\n"
        "--add-pov-feature, --add-normalized-log-pitch, --add-delta-pitch and --add-raw-log-pitch\n"
        "\n"
        "Usage: process-kaldi-pitch-feats [options...] <feat-rspecifier> <feats-wspecifier>\n"
        "\n"
        "e.g.: compute-kaldi-pitch-feats [args] ark:- | process-kaldi-pitch-feats ark:- ark:feats.ark\n");
    po.Register("pitch-scale", &o.pitch_scale, "Scaling factor for the final normalized log-pitch value");
    po.Register("pov-scale", &o.pov_scale, "Scaling factor for final POV (probability of voicing) feature");
    po.Register("pov-offset", &o.pov_offset, "This can be used to add an offset to the POV feature. Intended for use in online decoding as a substitute for  CMN.");
    po.Register("delta-pitch-scale", &o.delta_pitch_scale, "Term to scale the final delta log-pitch feature");
    po.Register("delta-pitch-noise-stddev", &o.delta_pitch_noise_stddev, "Standard deviation for noise we add to the delta log-pitch (before scaling); should be about the "
                                                                         "same as delta-pitch option to pitch creation.");
    po.Register("normalization-left-context", &o.normalization_left_context, "Left-context (in frames) for moving window normalization");
    po.Register("normalization-right-context", &o.normalization_right_context, "Right-context (in frames) for moving window normalization");
    po.Register("delta-window", &o.delta_window, "Number of frames on each side of central frame, to use for delta window.");
    po.Register("delay", &o.delay, "Number of frames by which the pitch information is delayed.");
    po.Register("add-pov-feature", &add_pov_feature, "If true, the warped NCCF is added to output features");
    po.Register("add-normalized-log-pitch", &add_normalized_log_pitch, "If true, the log-pitch with POV-weighted mean subtraction over 1.5 second window is added to output features");
    po.Register("add-delta-pitch", &add_delta_pitch, "If true, time derivative of log-pitch is added to output features");
    po.Register("add-raw-log-pitch", &add_raw_log_pitch, "If true, log(pitch) is added to output features");
    po.Register("noise-seed", &noise_seed, "Seed of the delta-pitch noise's counter-based generator (a seed reproduces its features)");
    po.Register("srand", &srand_seed, "Seed for random number generator [accepted and unused: see --noise-seed]");
    po.Register("device", &device, "GPU index");
    po.Read(argc, argv);
    if (po.NumArgs() != 2) {
      po.PrintUsage();
      return 1;
    }
    o.add_pov_feature = add_pov_feature; o.add_normalized_log_pitch = add_normalized_log_pitch; o.add_delta_pitch = add_delta_pitch;
    o.add_raw_log_pitch = add_raw_log_pitch; o.noise_seed = (unsigned long long)noise_seed;

    eesen_pitch_t* pt = nullptr;
    ck(eesen_pitch_create(device, nullptr, &o, &pt));
    int dim = 0;
    ck(eesen_pitch_shape(pt, 0, nullptr, nullptr, &dim));
    FeatureReader reader(po.GetArg(1));
    MatrixWriter writer(po.GetArg(2));
    const long kBatchFrames = 1L << 20;
    long num_done = 0, total = 0;
    std::vector<std::pair<std::string, Mat>> batch;
    std::vector<unsigned long long> ids;
    auto flush = [&]() {
      const int S = (int)batch.size();
      std::vector<const float*> raw(S);
      std::vector<int> frames(S);
      std::vector<long> cap(S);
      std::vector<std::vector<float>> out(S);
      std::vector<float*> outp(S);
      for (int s = 0; s < S; ++s) {
        raw[s] = batch[s].second.v.data();
        frames[s] = batch[s].second.rows;
        out[s].resize((size_t)(frames[s] + o.delay) * dim);
        outp[s] = out[s].data();
        cap[s] = (long)out[s].size();
      }
      ck(eesen_pitch_process(pt, raw.data(), frames.data(), ids.data(), S, outp.data(), cap.data(), nullptr));
      for (int s = 0; s < S; ++s) {
        writer.Write(batch[s].first, out[s].data(), frames[s] + o.delay, dim, dim);
        ++num_done;
      }
      batch.clear(); ids.clear(); total = 0;
    };
    for (; !reader.Done(); reader.Next()) {
      Mat& m = reader.Value();
      if (m.rows == 0) {
        std::cerr << "WARNING (process-kaldi-pitch-feats:main()) Empty matrix for utterance " << reader.Key() << ": producing no output." << std::endl;
        continue;
      }
      if (m.cols != 2) throw std::runtime_error("Input feature must be pitch feature (should have dimension 2): utterance " + reader.Key());
      if (!batch.empty() && total + m.rows > kBatchFrames) flush();
      total += m.rows;
      ids.push_back((unsigned long long)(reader.NumRead() - 1));   // the utterance's number in the table keys its noise
      batch.emplace_back(reader.Key(), std::move(m));
    }
    if (!batch.empty()) flush();
    std::cerr << "LOG (process-kaldi-pitch-feats:main()) Post-processed pitch for " << num_done << " utterances." << std::endl;
    eesen_pitch_destroy(pt);
    return num_done != 0 ? 0 : 1;
  } catch (const std::exception& e) {
    std::cerr << "ERROR (process-kaldi-pitch-feats:main()) " << e.what() << std::endl;
    return 255;
  }
}
