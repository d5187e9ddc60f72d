// compute_kaldi_pitch_feats.cc -- compute-kaldi-pitch-feats over the C-ABI: (NCCF, pitch) pairs from a wav table, on the device.
//
// Usage: compute-kaldi-pitch-feats [options...] <wav-rspecifier> <feats-wspecifier>
// The reference's tool (src/featbin/compute-kaldi-pitch-feats.cc) with every option name of PitchExtractionOptions::Register, its
// warnings and exit status (1 when nothing was done); a sample-rate mismatch is an error.  Utterances are batched by total samples
// and every batch is one minibatch of the device extractor (eesen_pitch_compute, INTEGRATION.md "Pitch").  Deviations: the options of
// online emulation (--frames-per-chunk, --simulate-first-pass-online, --nccf-ballast-online) and --preemphasis-coefficient are
// refused when set; a waveform too short for a frame gets the reference's warning and no matrix (the reference writes an empty one).
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
    bool nccf_ballast_online = false, simulate_first_pass_online = false, snip_edges = true;
    int device = 0;
    eesen_tools::ParseOptions po(
        "Apply Kaldi pitch extractor, starting from wav input.  Output is 2-dimensional\n"
        "features consisting of (NCCF, pitch in Hz), where NCCF is between -1 and 1, and\n"
        "higher for voiced frames.  You will typically pipe this into\n"
        "process-kaldi-pitch-feats.\n"
        "Usage: compute-kaldi-pitch-feats [options...] <wav-rspecifier> <feats-wspecifier>\n"
        "e.g.\n"
        "compute-kaldi-pitch-feats --sample-frequency=8000 scp:wav.scp ark:- \n");
    po.Register("sample-frequency", &o.samp_freq, "Waveform data sample frequency (must match the waveform file, if specified there)");
    po.Register("frame-length", &o.frame_length_ms, "Frame length in milliseconds");
    po.Register("frame-shift", &o.frame_shift_ms, "Frame shift in milliseconds");
    po.Register("preemphasis-coefficient", &o.preemph_coeff, "Coefficient for use in signal preemphasis (deprecated) [must be 0]");
    po.Register("min-f0", &o.min_f0, "min. F0 to search for (Hz)");
    po.Register("max-f0", &o.max_f0, "max. F0 to search for (Hz)");
    po.Register("soft-min-f0", &o.soft_min_f0, "Minimum f0, applied in soft way, must not exceed min-f0");
    po.Register("penalty-factor", &o.penalty_factor, "cost factor for FO change.");
    po.Register("lowpass-cutoff", &o.lowpass_cutoff, "cutoff frequency for LowPass filter (Hz) ");
    po.Register("resample-frequency", &o.resample_freq, "Frequency that we down-sample the signal to.  Must be more than twice lowpass-cutoff");
    po.Register("delta-pitch", &o.delta_pitch, "Smallest relative change in pitch that our algorithm measures");
    po.Register("nccf-ballast", &o.nccf_ballast, "Increasing this factor reduces NCCF for quiet frames");
    po.Register("nccf-ballast-online", &nccf_ballast_online, "This is useful mainly for debug; it affects how the NCCF ballast is computed. [not supported]");
    po.Register("lowpass-filter-width", &o.lowpass_filter_width, "Integer that determines filter width of lowpass filter, more gives sharper filter");
    po.Register("upsample-filter-width", &o.upsample_filter_width, "Integer that determines filter width when upsampling NCCF");
    po.Register("frames-per-chunk", &o.frames_per_chunk, "Only relevant for offline pitch extraction with online compatibility [not supported: must be 0]");
    po.Register("simulate-first-pass-online", &simulate_first_pass_online, "If true, output the features an online decoder would see in the first pass [not supported]");
    po.Register("recompute-frame", &o.recompute_frame, "The frame below which an utterance's NCCF is re-scaled once the whole signal's energy is known");
    po.Register("max-frames-latency", &o.max_frames_latency, "Maximum number of frames of latency that we allow pitch tracking to introduce (no effect offline)");
    po.Register("snip-edges", &snip_edges, "If this is set to false, the incomplete frames near the ending edge won't be snipped, so that the number of "
                                           "frames is the file size divided by the frame-shift. This makes different types of features give the same number of frames.");
    po.Register("device", &device, "GPU index");
    po.Read(argc, argv);
    if (po.NumArgs() != 2) {
      po.PrintUsage();
      return 1;
    }
    o.nccf_ballast_online = nccf_ballast_online; o.simulate_first_pass_online = simulate_first_pass_online; o.snip_edges = snip_edges;

    eesen_pitch_t* pt = nullptr;
    ck(eesen_pitch_create(device, nullptr, &o, &pt));
    WaveSelect sel;
    sel.samp_freq = o.samp_freq; sel.channel = -1; sel.min_duration = 0.f; sel.tool = "compute-kaldi-pitch-feats";
    FeatureReader reader(po.GetArg(1), &sel);
    MatrixWriter writer(po.GetArg(2));
    const long kBatchSamples = 1L << 22;   // 4 M samples per minibatch: 26 k frames of 16 kHz audio, 90 MB of NCCF rows on the device
    long num_done = 0, total = 0;
    std::vector<std::pair<std::string, Mat>> batch;
    auto flush = [&]() {
      const int S = (int)batch.size();
      std::vector<const float*> wav(S);
      std::vector<int> nsamp(S), frames(S);
      std::vector<long> cap(S);
      std::vector<std::vector<float>> out(S);
      std::vector<float*> outp(S);
      for (int s = 0; s < S; ++s) {
        wav[s] = batch[s].second.v.data();
        nsamp[s] = batch[s].second.rows;
        ck(eesen_pitch_shape(pt, nsamp[s], &frames[s], nullptr, nullptr));
        out[s].resize((size_t)frames[s] * 2);
        outp[s] = out[s].data();
        cap[s] = (long)out[s].size();
      }
      ck(eesen_pitch_compute(pt, wav.data(), nsamp.data(), nullptr, S, 0, outp.data(), cap.data(), nullptr));
      for (int s = 0; s < S; ++s) {
        if (frames[s] == 0) {
          std::cerr << "WARNING (compute-kaldi-pitch-feats:ComputeKaldiPitch()) No frames output in pitch extraction for utterance " << batch[s].first << std::endl;
          continue;
        }
        writer.Write(batch[s].first, out[s].data(), frames[s], 2, 2);
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
    std::cerr << "LOG (compute-kaldi-pitch-feats:main()) Done " << num_done << " utterances, 0 with errors." << std::endl;
    eesen_pitch_destroy(pt);
    return num_done != 0 ? 0 : 1;
  } catch (const std::exception& e) {
    std::cerr << "ERROR (compute-kaldi-pitch-feats:main()) " << e.what() << std::endl;
    return 255;
  }
}
