// paste_feats.cc -- paste-feats over the C-ABI: feature tables side by side, from audio on the device.
//
// Usage: paste-feats [options] <in-rspecifier1> <in-rspecifier2> [<in-rspecifier3> ...] <out-wspecifier>
//    or: paste-feats [options] <in-rxfilename1> <in-rxfilename2> [<in-rxfilename3> ...] <out-wxfilename>
// The reference's tool (src/featbin/paste-feats.cc) with its usage, warnings, "Done N utts, errors on M" and exit status.  Two paths.
// When the inputs are exactly the two pipes the tonal recipes paste (asr_egs/wsj/steps/make_fbank_pitch.sh:117-121)
//   "ark:compute-fbank-feats [options] <wav-rspecifier> ark:- |"
//   "ark,s,cs:compute-kaldi-pitch-feats [options] <wav-rspecifier> ark:- | process-kaldi-pitch-feats [options] ark:- ark:- |"
// (what feat_pipeline.h recognises as a paste-feats head) neither pipe is run: the wav table is read once, batched by total samples,
// and every batch is one pass of the feeder's EESEN_FEAT_FBANK_PITCH stage -- one upload, the filterbank, the pitch tracker and the
// join on the device, one copy back (INTEGRATION.md "Fbank + pitch").  Any other inputs are joined on the host and need no device:
// the first table is read sequentially, the others by key (a sorted table, ark,s: is walked forward; any other is read whole).
#include <iostream>
#include <map>
#include <memory>
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

static void length_warning(const std::vector<int>& frames, const std::string& utt, int tolerance) {
  int lo = frames[0], hi = frames[0];
  for (int f : frames) { lo = std::min(lo, f); hi = std::max(hi, f); }
  std::cerr << "WARNING (paste-feats:AppendFeats()) Length mismatch " << hi << " vs. " << lo << (utt.empty() ? "" : " for utt ") << utt
            << " exceeds tolerance " << tolerance << std::endl;
}

// AppendFeats (paste-feats.cc:30-65): false (and the warning) when the lengths differ by more than the tolerance or one is empty
static bool append_feats(const std::vector<const Mat*>& in, const std::string& utt, int tolerance, Mat* out) {
  std::vector<int> frames;
  int cols = 0;
  for (const Mat* m : in) { frames.push_back(m->rows); cols += m->cols; }
  int rows = 0;
  ck(eesen_feat_paste_frames(frames.data(), (int)frames.size(), tolerance, &rows));
  if (rows == 0) { length_warning(frames, utt, tolerance); return false; }
  out->rows = rows; out->cols = cols;
  out->v.resize((size_t)rows * cols);
  int at = 0;
  for (const Mat* m : in) {
    for (int r = 0; r < rows; ++r) std::copy(m->v.begin() + (size_t)r * m->cols, m->v.begin() + (size_t)(r + 1) * m->cols, out->v.begin() + (size_t)r * cols + at);
    at += m->cols;
  }
  return true;
}

// RandomAccessBaseFloatMatrixReader
class ByKey {
 public:
  explicit ByKey(const std::string& rspecifier) : reader_(rspecifier) {
    const std::string head = rspecifier.substr(0, rspecifier.find(':'));
    std::istringstream hs(head);
    std::vector<std::string> opts;
    for (std::string o; std::getline(hs, o, ',');) opts.push_back(o);
    for (size_t i = 1; i < opts.size(); ++i) if (opts[0] == "ark" && opts[i] == "s") sorted_ = true;
    if (!sorted_)
      for (; !reader_.Done(); reader_.Next()) table_[reader_.Key()] = std::move(reader_.Value());
  }
  const Mat* Get(const std::string& key) {
    if (!sorted_) {
      auto it = table_.find(key);
      return it == table_.end() ? nullptr : &it->second;
    }
    while (!reader_.Done() && reader_.Key() < key) reader_.Next();
    return !reader_.Done() && reader_.Key() == key ? &reader_.Value() : nullptr;
  }
 private:
  FeatureReader reader_;
  bool sorted_ = false;
  std::map<std::string, Mat> table_;
};

static std::string quoted(const std::string& s) {   // for feat_pipeline.h's shell_split; "" when neither quote can hold it
  if (s.find('"') == std::string::npos) return '"' + s + '"';
  if (s.find('\'') == std::string::npos) return '\'' + s + '\'';
  return "";
}

int main(int argc, char** argv) {
  try {
    int length_tolerance = 0, device = 0;
    bool binary = true;
    eesen_tools::ParseOptions po(
        "Paste feature files (assuming they have the same lengths);  think of the\n"
        "unix command paste a b.\n"
        "Usage: paste-feats <in-rspecifier1> <in-rspecifier2> [<in-rspecifier3> ...] <out-wspecifier>\n"
        " or: paste-feats <in-rxfilename1> <in-rxfilename2> [<in-rxfilename3> ...] <out-wxfilename>\n"
        " e.g. paste-feats ark:feats1.ark \"ark:select-feats 0-3 ark:feats2.ark ark:- |\" ark:feats-out.ark\n"
        "  or: paste-feats foo.mat bar.mat baz.mat\n"
        "See also: copy-feats, copy-matrix, append-vector-to-feats, concat-feats\n");
    po.Register("length-tolerance", &length_tolerance, "If length is different, trim as shortest up to a frame  difference of length-tolerance, otherwise exclude segment.");
    po.Register("binary", &binary, "If true, output files in binary (only relevant for single-file operation, i.e. no tables)");
    po.Register("device", &device, "GPU index (only when the inputs are the two recognised pipes from audio)");
    po.Read(argc, argv);
    if (po.NumArgs() < 3) {
      po.PrintUsage();
      return 1;
    }
    const int n_in = po.NumArgs() - 1;
    const std::string out_name = po.GetArg(po.NumArgs());
    if (!table_kind(po.GetArg(1))) {   // rxfilenames: one matrix each
      std::vector<Mat> mats(n_in);
      std::vector<const Mat*> ptrs;
      for (int i = 0; i < n_in; ++i) {
        std::string loc = po.GetArg(i + 1);
        std::streamoff off = 0;
        const size_t c = loc.rfind(':');
        if (loc.find('|') == std::string::npos && c != std::string::npos && c + 1 < loc.size() && loc.find_first_not_of("0123456789", c + 1) == std::string::npos) {
          off = std::stoll(loc.substr(c + 1));
          loc = loc.substr(0, c);
        }
        InStream in(loc);
        if (off) in.get().seekg(off);
        mats[i] = read_matrix(in.get());
        ptrs.push_back(&mats[i]);
      }
      Mat out;
      if (!append_feats(ptrs, "", length_tolerance, &out)) return 1;
      OutStream os(out_name);
      std::ostream& f = os.get();
      if (binary) {
        f.write("\0BFM ", 5);
        const char four = 4;
        const int32_t rc[2] = {out.rows, out.cols};
        for (int i = 0; i < 2; ++i) { f.write(&four, 1); f.write(reinterpret_cast<const char*>(&rc[i]), 4); }
        f.write(reinterpret_cast<const char*>(out.v.data()), out.v.size() * 4);
      } else {
        f << " [";
        f.precision(9);
        for (int r = 0; r < out.rows; ++r) {
          f << "\n  ";
          for (int c = 0; c < out.cols; ++c) f << out.v[(size_t)r * out.cols + c] << ' ';
        }
        f << "]\n";
      }
      f.flush();
      if (!f) throw std::runtime_error("write error");
      std::cerr << "LOG (paste-feats:main()) Wrote appended features to " << out_name << std::endl;
      return 0;
    }

    MatrixWriter writer(out_name);
    long num_done = 0, num_err = 0;
    Pipeline pipe;
    bool fused = false;
    if (n_in == 2) {
      const std::string a = quoted(po.GetArg(1)), b = quoted(po.GetArg(2));
      fused = !a.empty() && !b.empty() &&
              parse_feature_pipeline("ark:paste-feats --length-tolerance=" + std::to_string(length_tolerance) + " " + a + " " + b + " ark:- |", &pipe);
    }
    if (fused) {
      eesen_feeder_t* feeder = nullptr;
      ck(eesen_feeder_create(device, nullptr, 1, &feeder));
      ck(pipe.configure(feeder));
      eesen_fbank_t* fb = nullptr;      // the two counts of a dropped utterance's warning: host-only shape calls
      eesen_pitch_t* pt = nullptr;
      ck(eesen_fbank_create(device, nullptr, &pipe.fbank, &fb));
      ck(eesen_pitch_create(device, nullptr, &pipe.pitch, &pt));
      FeatureReader reader(pipe.source, pipe.wave_mode());
      const long kBatchSamples = 1L << 22;   // as compute-kaldi-pitch-feats: the pitch tracker's scratch is what bounds a batch
      long total = 0;
      std::vector<std::pair<std::string, Mat>> batch;
      std::vector<float> host;
      auto flush = [&]() {
        std::vector<const float*> wav;
        std::vector<int> nsamp, rows(batch.size()), col(batch.size(), -1);
        int cols = 0;
        for (size_t s = 0; s < batch.size(); ++s) {
          ck(eesen_feeder_pipeline_shape(feeder, 1, batch[s].second.rows, &cols, &rows[s]));
          if (!rows[s]) continue;
          col[s] = (int)wav.size();
          wav.push_back(batch[s].second.v.data());
          nsamp.push_back(batch[s].second.rows);
        }
        int T = 0, S = 0, ld = 0;
        if (!wav.empty()) {
          int slot = -1;
          float* dev = nullptr;
          ck(eesen_feeder_submit_raw(feeder, wav.data(), nsamp.data(), nullptr, nullptr, (int)wav.size(), 1, &slot));
          ck(eesen_feeder_acquire(feeder, slot, &dev, &T, &S, &ld));
          host.resize((size_t)T * S * ld);
          ck(eesen_dev_copy(device, host.data(), dev, (long)host.size() * 4, 2));
          ck(eesen_feeder_release(feeder, slot));
        }
        for (size_t s = 0; s < batch.size(); ++s) {
          if (!rows[s]) {
            int f = 0, p = 0;
            ck(eesen_fbank_shape(fb, batch[s].second.rows, &f, nullptr));
            ck(eesen_pitch_shape(pt, batch[s].second.rows, &p, nullptr, nullptr));
            length_warning({f, p ? p + pipe.pitch.delay : 0}, batch[s].first, length_tolerance);
            ++num_err;
            continue;
          }
          writer.Write(batch[s].first, host.data() + (size_t)col[s] * ld, rows[s], cols, S * ld);   // row t of utterance s is row t * S + s
          ++num_done;
        }
        batch.clear(); total = 0;
      };
      for (; !reader.Done(); reader.Next()) {
        Mat& m = reader.Value();
        if (!batch.empty() && total + m.rows > kBatchSamples) flush();
        total += m.rows;
        batch.emplace_back(reader.Key(), std::move(m));
      }
      if (!batch.empty()) flush();
      eesen_pitch_destroy(pt);
      eesen_fbank_destroy(fb);
      eesen_feeder_destroy(feeder);
    } else {
      FeatureReader input1(po.GetArg(1));
      std::vector<std::unique_ptr<ByKey>> input;
      for (int i = 2; i <= n_in; ++i) input.emplace_back(new ByKey(po.GetArg(i)));
      for (; !input1.Done(); input1.Next()) {
        const std::string utt = input1.Key();
        std::vector<const Mat*> feats{&input1.Value()};
        size_t i = 0;
        for (; i < input.size(); ++i) {
          const Mat* m = input[i]->Get(utt);
          if (!m) {
            std::cerr << "WARNING (paste-feats:main()) Missing utt " << utt << " from input " << po.GetArg((int)i + 2) << std::endl;
            ++num_err;
            break;
          }
          feats.push_back(m);
        }
        if (i != input.size()) continue;
        Mat out;
        if (!append_feats(feats, utt, length_tolerance, &out)) { ++num_err; continue; }
        writer.Write(utt, out.v.data(), out.rows, out.cols, out.cols);
        ++num_done;
      }
    }
    std::cerr << "LOG (paste-feats:main()) Done " << num_done << " utts, errors on " << num_err << std::endl;
    return num_done == 0 ? 255 : 0;
  } catch (const std::exception& e) {
    std::cerr << "ERROR (paste-feats:main()) " << e.what() << std::endl;
    return 255;
  }
}
