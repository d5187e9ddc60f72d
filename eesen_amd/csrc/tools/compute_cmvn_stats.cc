// compute_cmvn_stats.cc -- compute-cmvn-stats over the C-ABI: CMVN statistics per utterance, per speaker or global, on the device.
//
// Usage: compute-cmvn-stats  [options] feats-rspecifier (stats-wspecifier|stats-wxfilename)
// The reference's tool (src/featbin/compute-cmvn-stats.cc) with its options, three modes, warnings, final log line and exit status
// (0 if and only if an utterance was accumulated).  One sequential pass over the feature rspecifier: utterances are batched by total
// floats and every batch is one call (eesen_cmvn_stats_parallel), or, where the rspecifier is a pipe the front end recognises
// (feat_pipeline.h: `ark:compute-fbank-feats ... scp:wav.scp ark:- |`, the paste-feats head, such a head or a table behind recognised
// filters), a feeder pipeline with the statistics tap on its last boundary, so the features never come back to the host.  The
// 2 x (D+1) doubles of every utterance are kept; speakers are summed on the host in fp64 in the order of each spk2utt list, the global
// matrix in table order and rounded to float once.  Deviations: --device is new; --weights with a pipeline rspecifier is refused (the
// tap is unweighted); --spk2utt reads the features sequentially, so an utterance listed twice in the table counts as its last entry.
#include <iostream>
#include <map>
#include <string>
#include <vector>

#include "../../../include/eesen_hip.h"
#include "feat_pipeline.h"
#include "kaldi_tables.h"
#include "parse_options.h"

using namespace ktab;

static void ck(int rc) {
  if (rc != EESEN_OK) throw std::runtime_error(eesen_last_error());
}
static const char* kWarn = "WARNING (compute-cmvn-stats:main()) ";

// ClassifyWspecifier (src/util/kaldi-table.cc): options in front of the first ':' with `ark` or `scp` among them
static bool is_wspecifier(const std::string& s) {
  const size_t colon = s.find(':');
  if (colon == std::string::npos) return false;
  bool table = false;
  std::istringstream hs(s.substr(0, colon));
  for (std::string o; std::getline(hs, o, ',');) {
    if (o == "ark" || o == "scp") table = true;
    else if (o != "t" && o != "b" && o != "f" && o != "nf" && o != "p") return false;
  }
  return table;
}

enum { kOk = 0, kNoWeights = 1, kBadWeights = 2 };
struct UttStats {
  std::string key;
  int status = kOk, dim = 0, rows = 0, wdim = 0;
  std::vector<double> stats;   // [2 x (dim + 1)]
};

int main(int argc, char** argv) {
  try {
    std::string spk2utt, weights_rspecifier;
    bool binary = true;
    int device = 0;
    eesen_tools::ParseOptions po(
        "Compute cepstral mean and variance normalization statistics\n"
        "If wspecifier provided: per-utterance by default, or per-speaker if\n"
        "spk2utt option provided; if wxfilename: global\n"
        "Usage: compute-cmvn-stats  [options] feats-rspecifier (stats-wspecifier|stats-wxfilename)\n");
    po.Register("spk2utt", &spk2utt, "rspecifier for speaker to utterance-list map");
    po.Register("binary", &binary, "write in binary mode (applies only to global CMN/CVN)");
    po.Register("weights", &weights_rspecifier, "rspecifier for a vector of floats for each utterance, that's a per-frame weight.");
    po.Register("device", &device, "GPU index");
    po.Read(argc, argv);
    if (po.NumArgs() != 2) {
      po.PrintUsage();
      return 1;
    }
    const std::string rspecifier = po.GetArg(1), out_name = po.GetArg(2);
    const bool to_table = is_wspecifier(out_name);
    if (!to_table && !spk2utt.empty())
      throw std::runtime_error("--spk2utt option not compatible with wxfilename as output (did you forget ark:?)");
    Pipeline pipe;
    const bool piped = !getenv("EESEN_HOST_FEATURE_PIPES") && parse_feature_pipeline(rspecifier, &pipe);
    if (piped && !weights_rspecifier.empty())
      throw std::runtime_error("--weights is not supported with a feature pipeline computed on the device (the statistics tap is unweighted): "
                               "write the features to an archive first");
    const bool weighted = !weights_rspecifier.empty();
    std::map<std::string, std::vector<float>> weights;
    if (weighted) weights = read_float_vectors(weights_rspecifier);

    // ---- the one pass: every utterance's statistics, in table order
    std::vector<UttStats> utts;
    std::vector<std::pair<std::string, Mat>> batch;
    std::vector<size_t> place;   // of the batch's utterances in `utts`
    std::vector<const float*> cmvn;
    long total = 0;
    eesen_feeder_t* feeder = nullptr;
    std::unique_ptr<CmvnTable> cmvn_table;
    if (piped) {
      ck(eesen_feeder_create(device, nullptr, 2, &feeder));
      ck(pipe.configure(feeder));
      ck(eesen_feeder_set_stats_tap(feeder, (int)pipe.stages.size()));
      if (!pipe.cmvn.empty()) cmvn_table.reset(new CmvnTable(pipe.cmvn, pipe.utt2spk, pipe.norm_vars));
    }
    std::vector<double> buf;
    auto flush = [&]() {
      const int S = (int)batch.size();
      std::vector<const float*> ptr(S), wptr(S, nullptr);
      std::vector<int> frames(S);
      for (int s = 0; s < S; ++s) { ptr[s] = batch[s].second.v.data(); frames[s] = batch[s].second.rows; }
      int D = batch[0].second.cols;
      if (piped) {
        int slot = 0, Din = D;
        ck(eesen_feeder_pipeline_shape(feeder, Din, 1, &D, nullptr));
        buf.assign((size_t)S * 2 * (D + 1), 0.0);
        ck(eesen_feeder_submit_raw(feeder, ptr.data(), frames.data(), nullptr, cmvn_table ? cmvn.data() : nullptr, S, Din, &slot));
        int Dt = 0;
        ck(eesen_feeder_stats(feeder, slot, buf.data(), &Dt));
        if (Dt != D) throw std::runtime_error("the statistics tap answered for another dimension");
      } else {
        if (weighted)
          for (int s = 0; s < S; ++s) wptr[s] = weights[batch[s].first].data();
        buf.assign((size_t)S * 2 * (D + 1), 0.0);
        ck(eesen_cmvn_stats_parallel(device, nullptr, ptr.data(), frames.data(), nullptr, weighted ? wptr.data() : nullptr, S, D, buf.data()));
      }
      const size_t n = (size_t)2 * (D + 1);
      for (int s = 0; s < S; ++s) {
        UttStats& u = utts[place[s]];
        u.dim = D;
        u.stats.assign(buf.begin() + s * n, buf.begin() + (s + 1) * n);
      }
      batch.clear(); place.clear(); cmvn.clear(); total = 0;
    };
    const long kBatchFloats = 1L << 23;   // 8 M floats (32 MB) per launch, as compute-fbank-feats batches its samples
    {
      FeatureReader reader(piped ? pipe.source : rspecifier, piped ? pipe.wave_mode() : nullptr);
      for (; !reader.Done(); reader.Next()) {
        Mat& m = reader.Value();
        const std::string utt = reader.Key();
        const float* cm = nullptr;
        if (piped) {   // what the extractor and the filters would have dropped
          if (cmvn_table) {
            const std::vector<float>* nm = cmvn_table->lookup(utt);
            if (!nm) { std::cerr << kWarn << "No normalization statistics available for key " << utt << ", producing no output for this utterance" << std::endl; continue; }
            if (CmvnTable::dim(*nm) != pipe.cmvn_dim(m.cols))
              throw std::runtime_error("Dim mismatch in ApplyCmvn: cmvn 2x" + std::to_string(CmvnTable::dim(*nm) + 1) + ", feats " + std::to_string(m.rows) + "x" + std::to_string(m.cols));
            cm = nm->data();
          }
          int rows = 0, cols = 0;
          if (m.rows > 0 && m.cols > 0) ck(eesen_feeder_pipeline_shape(feeder, m.cols, m.rows, &cols, &rows));
          if (rows == 0) {
            std::cerr << kWarn << (pipe.has_fbank ? "Failed to compute features for utterance " : "Empty feature matrix for utterance ") << utt << std::endl;
            continue;
          }
        }
        UttStats u;
        u.key = utt; u.dim = m.cols; u.rows = m.rows;
        if (weighted) {
          auto w = weights.find(utt);
          if (w == weights.end()) u.status = kNoWeights;
          else if ((int)w->second.size() != m.rows) { u.status = kBadWeights; u.wdim = (int)w->second.size(); }
        }
        utts.push_back(u);
        if (u.status != kOk) continue;
        if (m.cols <= 0) throw std::runtime_error("feature matrix without columns for utterance " + utt);
        // a batch holds matrices of one width
        if (!batch.empty() && (total + (long)m.v.size() > kBatchFloats || batch[0].second.cols != m.cols || (int)batch.size() == 65535)) flush();
        total += (long)m.v.size();
        cmvn.push_back(cm);
        place.push_back(utts.size() - 1);
        batch.emplace_back(utt, std::move(m));
      }
      if (!batch.empty()) flush();
    }
    if (feeder) eesen_feeder_destroy(feeder);

    // ---- the three modes over the kept matrices
    long num_done = 0, num_err = 0;
    auto usable = [&](const UttStats& u) {   // AccCmvnStatsWrapper's two warnings
      if (u.status == kNoWeights) std::cerr << kWarn << "No weights available for utterance " << u.key << std::endl;
      if (u.status == kBadWeights) std::cerr << kWarn << "Weights for utterance " << u.key << " have wrong dimension " << u.wdim << " vs. " << u.rows << std::endl;
      return u.status == kOk;
    };
    auto add = [](std::vector<double>* acc, const UttStats& u) {
      if (acc->size() != (size_t)2 * (u.dim + 1)) throw std::runtime_error("feature dimension of utterance " + u.key + " differs from the statistics it is added to");
      if (u.status == kOk) for (size_t i = 0; i < acc->size(); ++i) (*acc)[i] += u.stats[i];
    };
    if (to_table) {
      DoubleMatrixWriter writer(out_name);
      if (!spk2utt.empty()) {
        std::map<std::string, size_t> index;
        for (size_t i = 0; i < utts.size(); ++i) index[utts[i].key] = i;
        for (const auto& spk : read_token_lists(spk2utt)) {
          std::vector<double> acc;
          int dim = 0;
          for (const std::string& utt : spk.second) {
            auto it = index.find(utt);
            if (it == index.end()) {
              std::cerr << kWarn << "Did not find features for utterance " << utt << std::endl;
              ++num_err;
              continue;
            }
            const UttStats& u = utts[it->second];
            if (acc.empty()) { dim = u.dim; acc.assign((size_t)2 * (dim + 1), 0.0); }   // InitCmvnStats on the first utterance found
            add(&acc, u);
            if (usable(u)) ++num_done; else ++num_err;
          }
          if (acc.empty()) std::cerr << kWarn << "No stats accumulated for speaker " << spk.first << std::endl;
          else writer.Write(spk.first, acc.data(), 2, dim + 1);
        }
      } else {
        for (const UttStats& u : utts) {
          if (!usable(u)) { ++num_err; continue; }
          writer.Write(u.key, u.stats.data(), 2, u.dim + 1);
          ++num_done;
        }
      }
    } else {
      std::vector<double> acc;
      int dim = 0;
      for (const UttStats& u : utts) {
        if (acc.empty()) { dim = u.dim; acc.assign((size_t)2 * (dim + 1), 0.0); }
        add(&acc, u);
        if (usable(u)) ++num_done; else ++num_err;
      }
      std::vector<float> f(acc.begin(), acc.end());   // Matrix<float> stats_float(stats): rounded once
      OutStream out(out_name);   // (a run without an utterance writes the reference's empty matrix)
      if (!binary && acc.empty()) out.get() << " [ ]\n";
      else write_matrix_body(out.get(), !binary, f.data(), acc.empty() ? 0 : 2, acc.empty() ? 0 : dim + 1, dim + 1, 7);
      out.get().flush();
      if (!out.get()) throw std::runtime_error("write error");
      std::cerr << "LOG (compute-cmvn-stats:main()) Wrote global CMVN stats to " << (out_name == "-" ? "standard output" : out_name) << std::endl;
    }
    std::cerr << "LOG (compute-cmvn-stats:main()) Done accumulating CMVN stats for " << num_done << " utterances; " << num_err << " had errors." << std::endl;
    return num_done != 0 ? 0 : 1;
  } catch (const std::exception& e) {
    std::cerr << "ERROR (compute-cmvn-stats:main()) " << e.what() << std::endl;
    return 255;
  }
}
