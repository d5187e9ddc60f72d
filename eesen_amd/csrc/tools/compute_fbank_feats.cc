// compute_fbank_feats.cc -- compute-fbank-feats over the C-ABI: log-mel filterbank features from a wav table, on the device.
//
// Usage:  compute-fbank-feats [options...] <wav-rspecifier> <feats-wspecifier>
// The reference's tool (src/featbin/compute-fbank-feats.cc) with its option names, defaults, warnings and exit status (1 when nothing
// succeeded); utterances are batched by total samples and every batch is one launch (eesen_fbank_compute, INTEGRATION.md "Fbank").
// Deviations: --dither-seed is new (the dither is a counter-based generator keyed by seed, utterance number, frame and sample, so a run
// reproduces; --dither=0 is the path held to the reference); --vtln-map, --utt2spk, --output-format=htk and
// --round-to-power-of-two=false are refused.
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
    eesen_fbank_opts_t fo;
    eesen_fbank_opts_default(&fo);
    bool remove_dc_offset = true, round_to_power_of_two = true, snip_edges = true, use_energy = false, raw_energy = true, htk_compat = false,
         use_log_fbank = true, subtract_mean = false;
    std::string window_type = "povey", vtln_map, utt2spk, output_format = "kaldi";
    int channel = -1, device = 0, dither_seed = 0;
    float min_duration = 0.f;
    eesen_tools::ParseOptions po(
        "Create Mel-filter bank (FBANK) feature files.\n"
        "Usage:  compute-fbank-feats [options...] <wav-rspecifier> <feats-wspecifier>\n");
    po.Register("sample-frequency", &fo.samp_freq, "Waveform data sample frequency (must match the waveform file, if specified there)");
    po.Register("frame-length", &fo.frame_length_ms, "Frame length in milliseconds");
    po.Register("frame-shift", &fo.frame_shift_ms, "Frame shift in milliseconds");
    po.Register("preemphasis-coefficient", &fo.preemph_coeff, "Coefficient for use in signal preemphasis");
    po.Register("remove-dc-offset", &remove_dc_offset, "Subtract mean from waveform on each frame");
    po.Register("dither", &fo.dither, "Dithering constant (0.0 means no dither)");
    po.Register("window-type", &window_type, "Type of window (\"hamming\"|\"hanning\"|\"povey\"|\"rectangular\")");
    po.Register("round-to-power-of-two", &round_to_power_of_two, "If true, round window size to power of two.");
    po.Register("snip-edges", &snip_edges, "If true, end effects will be handled by outputting only frames that completely fit in the file, and the "
                                           "number of frames depends on the frame-length.  If false, the number of frames depends only on the "
                                           "frame-shift, and we reflect the data at the ends.");
    po.Register("num-mel-bins", &fo.num_bins, "Number of triangular mel-frequency bins");
    po.Register("low-freq", &fo.low_freq, "Low cutoff frequency for mel bins");
    po.Register("high-freq", &fo.high_freq, "High cutoff frequency for mel bins (if < 0, offset from Nyquist)");
    po.Register("vtln-low", &fo.vtln_low, "Low inflection point in piecewise linear VTLN warping function");
    po.Register("vtln-high", &fo.vtln_high, "High inflection point in piecewise linear VTLN warping function (if negative, offset from high-mel-freq");
    po.Register("use-energy", &use_energy, "Add an extra dimension with energy to the FBANK output.");
    po.Register("energy-floor", &fo.energy_floor, "Floor on energy (absolute, not relative) in FBANK computation");
    po.Register("raw-energy", &raw_energy, "If true, compute energy before preemphasis and windowing");
    po.Register("htk-compat", &htk_compat, "If true, put energy last.  Warning: not sufficient to get HTK compatible features (need to change other parameters).");
    po.Register("use-log-fbank", &use_log_fbank, "If true, produce log-filterbank, else produce linear.");
    po.Register("vtln-warp", &fo.vtln_warp, "Vtln warp factor (only applicable if vtln-map not specified)");
    po.Register("dither-seed", &dither_seed, "Seed of the dither's counter-based generator (a seed reproduces its features)");
    po.Register("subtract-mean", &subtract_mean, "Subtract mean of each feature file [CMS]; not recommended to do it this way. ");
    po.Register("vtln-map", &vtln_map, "Map from utterance or speaker-id to vtln warp factor (rspecifier) [not supported]");
    po.Register("utt2spk", &utt2spk, "Utterance to speaker-id map (if doing VTLN and you have warps per speaker) [not supported]");
    po.Register("channel", &channel, "Channel to extract (-1 -> expect mono, 0 -> left, 1 -> right)");
    po.Register("min-duration", &min_duration, "Minimum duration of segments to process (in seconds).");
    po.Register("output-format", &output_format, "Format of the output files [kaldi only]");
    po.Register("device", &device, "GPU index");
    po.Read(argc, argv);
    if (po.NumArgs() != 2) {
      po.PrintUsage();
      return 1;
    }
    if (!vtln_map.empty() || !utt2spk.empty()) throw std::runtime_error("--vtln-map / --utt2spk are not supported: one --vtln-warp per run");
    if (output_format != "kaldi") throw std::runtime_error("--output-format=" + output_format + " is not supported (kaldi only)");
    fo.remove_dc_offset = remove_dc_offset; fo.round_to_power_of_two = round_to_power_of_two; fo.snip_edges = snip_edges;
    fo.use_energy = use_energy; fo.raw_energy = raw_energy; fo.htk_compat = htk_compat; fo.use_log_fbank = use_log_fbank;
    fo.dither_seed = (unsigned long long)dither_seed;
    const char* windows[] = {"hamming", "hanning", "povey", "rectangular"};
    fo.window_type = -1;
    for (int i = 0; i < 4; ++i) if (window_type == windows[i]) fo.window_type = i;
    if (fo.window_type < 0) throw std::runtime_error("Invalid window type " + window_type);

    eesen_fbank_t* fb = nullptr;
    ck(eesen_fbank_create(device, nullptr, &fo, &fb));
    WaveSelect sel;
    sel.samp_freq = fo.samp_freq; sel.channel = channel; sel.min_duration = min_duration;
    FeatureReader reader(po.GetArg(1), &sel);
    MatrixWriter writer(po.GetArg(2));
    const long kBatchSamples = 1L << 23;   // 8 M samples (32 MB of floats, nine minutes of 16 kHz audio) per launch
    long num_success = 0, total = 0;
    std::vector<std::pair<std::string, Mat>> batch;
    std::vector<unsigned long long> ids;
    auto flush = [&]() {
      const int S = (int)batch.size();
      std::vector<const float*> wav(S);
      std::vector<int> nsamp(S), frames(S);
      std::vector<std::vector<float>> out(S);
      std::vector<float*> outp(S);
      int dim = 0;
      for (int s = 0; s < S; ++s) {
        wav[s] = batch[s].second.v.data();
        nsamp[s] = batch[s].second.rows;
        ck(eesen_fbank_shape(fb, nsamp[s], &frames[s], &dim));
        out[s].resize((size_t)frames[s] * dim);
        outp[s] = out[s].data();
      }
      ck(eesen_fbank_compute(fb, wav.data(), nsamp.data(), ids.data(), S, outp.data()));
      for (int s = 0; s < S; ++s) {
        if (frames[s] == 0) {                 // (the reference fails on a waveform shorter than a frame)
          std::cerr << "WARNING (compute-fbank-feats:main()) Failed to compute features for utterance " << batch[s].first << std::endl;
          continue;
        }
        if (subtract_mean) {                  // compute-fbank-feats.cc:150-156, on the host behind the copy back
          for (int c = 0; c < dim; ++c) {
            float sum = 0.f;
            for (int r = 0; r < frames[s]; ++r) sum += out[s][(size_t)r * dim + c];
            const float mean = sum * (1.0f / frames[s]);
            for (int r = 0; r < frames[s]; ++r) out[s][(size_t)r * dim + c] -= mean;
          }
        }
        writer.Write(batch[s].first, out[s].data(), frames[s], dim, dim);
        ++num_success;
      }
      batch.clear(); ids.clear(); total = 0;
    };
    for (; !reader.Done(); reader.Next()) {
      Mat& m = reader.Value();
      if (!batch.empty() && total + m.rows > kBatchSamples) flush();
      total += m.rows;
      ids.push_back((unsigned long long)(reader.NumRead() - 1));   // the utterance's number in the table keys its dither
      batch.emplace_back(reader.Key(), std::move(m));
    }
    if (!batch.empty()) flush();
    const long num_utts = reader.NumRead();
    std::cerr << "LOG (compute-fbank-feats:main())  Done " << num_success << " out of " << num_utts << " utterances." << std::endl;
    eesen_fbank_destroy(fb);
    return num_success != 0 ? 0 : 1;
  } catch (const std::exception& e) {
    std::cerr << "ERROR (compute-fbank-feats:main()) " << e.what() << std::endl;
    return 255;
  }
}
