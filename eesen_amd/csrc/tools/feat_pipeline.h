// feat_pipeline.h -- host side of the device feature front end (include/eesen_hip.h, eesen_feeder_set_pipeline), shared by
// train_ctc_parallel.cc and net_output_extract.cc.
//
// The recipes hand both tools their features as an rspecifier that is a pipe of the reference's own filters
// (asr_egs/wsj/steps/train_ctc_parallel.sh:95-110, decode_ctc_lat.sh:92-95, librispeech/steps/train_ctc_parallel_mult.sh:110-133):
//   ark,s,cs:apply-cmvn --norm-vars=true --utt2spk=ark:data/utt2spk scp:data/cmvn.scp scp:exp/train.scp ark:- |
//            splice-feats --left-context=1 --right-context=1 ark:- ark:- | subsample-feats --n=3 --offset=0 ark:- ark:- | add-deltas ark:- ark:- |
// parse_feature_pipeline recognises exactly such command lines (the option sets of src/featbin/{apply-cmvn,copy-feats,splice-feats,
// subsample-feats,add-deltas}.cc); the tool then reads the RAW table itself, looks the CMVN statistics up per utterance, and the
// filters run on the GPU inside the batch assembly.  Anything else (another tool, an option not implemented, e.g. --skip-dims)
// is left to the shell: the rspecifier is opened as the pipe it is.  Same logic as eesen_amd/frontend.py.
//
// The pipe may start at the audio: `compute-fbank-feats [options] scp:wav.scp ark:- | apply-cmvn ... ark:- ark:- | add-deltas ark:- ark:- |`.
// The tool then reads the wav table itself (FeatureReader in wave mode) and the features are computed on the device as well
// (EESEN_FEAT_FBANK, the head stage); an option the device extractor does not implement (--vtln-map, --subtract-mean, htk output,
// --round-to-power-of-two=false ...) leaves the rspecifier unrecognised.
//
// Or at the audio through both extractors, the tonal recipes' features (asr_egs/wsj/steps/make_fbank_pitch.sh:117-121):
//   paste-feats --length-tolerance=2 "ark:compute-fbank-feats [options] scp,p:wav.scp ark:- |"
//               "ark,s,cs:compute-kaldi-pitch-feats [options] scp,p:wav.scp ark:- | process-kaldi-pitch-feats [options] ark:- ark:- |" ark:- | ...
// Both inner pipes must name the same wav table and every option must be one of the device extractors' (--config files are read as
// the tools read them); the head stage is then EESEN_FEAT_FBANK_PITCH.  The inputs in the other order, a third input, --binary or
// extract-segments leave the rspecifier unrecognised.
#pragma once
#include <cmath>
#include <fstream>
#include <map>
#include <string>
#include <vector>

#include "../../../include/eesen_hip.h"
#include "kaldi_tables.h"

namespace ktab {

struct Pipeline {
  std::string source;                       // rspecifier of the raw features
  std::vector<eesen_feat_stage_t> stages;   // in order
  std::string cmvn, utt2spk;                // statistics rspecifier / rxfilename ("" = no CMVN stage), utt2spk rspecifier
  bool norm_vars = false;
  // with a compute-fbank-feats head: `source` is the wav table
  bool has_fbank = false;
  eesen_fbank_opts_t fbank;
  WaveSelect wave;
  // with a paste-feats head over compute-fbank-feats and the two pitch tools: the pitch options and paste-feats' --length-tolerance
  bool has_pitch = false;
  eesen_pitch_opts_t pitch;
  int tolerance = 0;
  const WaveSelect* wave_mode() const { return has_fbank ? &wave : nullptr; }
  int pitch_dim() const { return (pitch.add_pov_feature != 0) + (pitch.add_normalized_log_pitch != 0) + (pitch.add_delta_pitch != 0) + (pitch.add_raw_log_pitch != 0); }
  int cmvn_dim(int raw_cols) const {   // in front of the CMVN stage
    return has_fbank ? fbank.num_bins + (fbank.use_energy ? 1 : 0) + (has_pitch ? pitch_dim() : 0) : raw_cols;
  }
  int configure(eesen_feeder_t* feeder) const {   // the extractors' options first, then the stages
    if (has_fbank) { const int rc = eesen_feeder_set_fbank(feeder, &fbank); if (rc != EESEN_OK) return rc; }
    if (has_pitch) { const int rc = eesen_feeder_set_pitch(feeder, &pitch); if (rc != EESEN_OK) return rc; }
    return eesen_feeder_set_pipeline(feeder, stages.data(), (int)stages.size());
  }
};

inline bool shell_split(const std::string& s, std::vector<std::string>* out) {  // whitespace-separated words, '...' and "..." quoting
  out->clear();
  std::string cur;
  bool have = false;
  for (size_t i = 0; i < s.size(); ++i) {
    const char c = s[i];
    if (c == '\'' || c == '"') {
      const size_t e = s.find(c, i + 1);
      if (e == std::string::npos) return false;
      cur += s.substr(i + 1, e - i - 1);
      have = true;
      i = e;
    } else if (c == ' ' || c == '\t' || c == '\n') {
      if (have) { out->push_back(cur); cur.clear(); have = false; }
    } else {
      cur += c;
      have = true;
    }
  }
  if (have) out->push_back(cur);
  return true;
}

inline bool to_bool(const std::string& v, bool* b) {  // ParseOptions::ToBool (src/util/parse-options.cc)
  std::string l;
  for (char c : v) l += (char)tolower(c);
  if (l.empty() || l == "true" || l == "t" || l == "1") { *b = true; return true; }
  if (l == "false" || l == "f" || l == "0") { *b = false; return true; }
  return false;
}
inline bool to_int(const std::string& v, int* x) {
  if (v.empty()) return false;
  char* end = nullptr;
  const long r = strtol(v.c_str(), &end, 10);
  if (*end) return false;
  *x = (int)r;
  return true;
}

inline bool to_float(const std::string& v, float* x) {
  if (v.empty()) return false;
  char* end = nullptr;
  const double r = strtod(v.c_str(), &end);
  if (*end) return false;
  *x = (float)r;
  return true;
}

// compute-fbank-feats' options onto eesen_fbank_opts_t (FrameExtractionOptions / MelBanksOptions / FbankOptions::Register, --vtln-warp of
// the tool, --dither-seed of this project); false: an unknown name or a value that does not parse
inline bool set_fbank_option(const std::string& name, const std::string& v, eesen_fbank_opts_t* o) {
  auto b = [&](int* dst) { bool x; if (!to_bool(v, &x)) return false; *dst = x ? 1 : 0; return true; };
  if (name == "sample-frequency") return to_float(v, &o->samp_freq);
  if (name == "frame-length") return to_float(v, &o->frame_length_ms);
  if (name == "frame-shift") return to_float(v, &o->frame_shift_ms);
  if (name == "preemphasis-coefficient") return to_float(v, &o->preemph_coeff);
  if (name == "remove-dc-offset") return b(&o->remove_dc_offset);
  if (name == "dither") return to_float(v, &o->dither);
  if (name == "window-type") {
    const char* names[] = {"hamming", "hanning", "povey", "rectangular"};
    for (int i = 0; i < 4; ++i) if (v == names[i]) { o->window_type = i; return true; }
    return false;
  }
  if (name == "round-to-power-of-two") return b(&o->round_to_power_of_two);
  if (name == "snip-edges") return b(&o->snip_edges);
  if (name == "num-mel-bins") return to_int(v, &o->num_bins);
  if (name == "low-freq") return to_float(v, &o->low_freq);
  if (name == "high-freq") return to_float(v, &o->high_freq);
  if (name == "vtln-low") return to_float(v, &o->vtln_low);
  if (name == "vtln-high") return to_float(v, &o->vtln_high);
  if (name == "use-energy") return b(&o->use_energy);
  if (name == "energy-floor") return to_float(v, &o->energy_floor);
  if (name == "raw-energy") return b(&o->raw_energy);
  if (name == "htk-compat") return b(&o->htk_compat);
  if (name == "use-log-fbank") return b(&o->use_log_fbank);
  if (name == "vtln-warp") return to_float(v, &o->vtln_warp);
  if (name == "dither-seed") {
    if (v.empty()) return false;
    char* end = nullptr;
    o->dither_seed = strtoull(v.c_str(), &end, 10);
    return !*end;
  }
  return false;
}

// compute-kaldi-pitch-feats' (which = 0: PitchExtractionOptions::Register) or process-kaldi-pitch-feats' (which = 1:
// ProcessPitchOptions::Register, plus --noise-seed of this project) options onto eesen_pitch_opts_t
inline bool set_pitch_option(int which, const std::string& name, const std::string& v, eesen_pitch_opts_t* o) {
  auto b = [&](int* dst) { bool x; if (!to_bool(v, &x)) return false; *dst = x ? 1 : 0; return true; };
  if (which == 0) {
    if (name == "sample-frequency") return to_float(v, &o->samp_freq);
    if (name == "frame-length") return to_float(v, &o->frame_length_ms);
    if (name == "frame-shift") return to_float(v, &o->frame_shift_ms);
    if (name == "preemphasis-coefficient") return to_float(v, &o->preemph_coeff);
    if (name == "min-f0") return to_float(v, &o->min_f0);
    if (name == "max-f0") return to_float(v, &o->max_f0);
    if (name == "soft-min-f0") return to_float(v, &o->soft_min_f0);
    if (name == "penalty-factor") return to_float(v, &o->penalty_factor);
    if (name == "lowpass-cutoff") return to_float(v, &o->lowpass_cutoff);
    if (name == "resample-frequency") return to_float(v, &o->resample_freq);
    if (name == "delta-pitch") return to_float(v, &o->delta_pitch);
    if (name == "nccf-ballast") return to_float(v, &o->nccf_ballast);
    if (name == "nccf-ballast-online") return b(&o->nccf_ballast_online);
    if (name == "lowpass-filter-width") return to_int(v, &o->lowpass_filter_width);
    if (name == "upsample-filter-width") return to_int(v, &o->upsample_filter_width);
    if (name == "frames-per-chunk") return to_int(v, &o->frames_per_chunk);
    if (name == "simulate-first-pass-online") return b(&o->simulate_first_pass_online);
    if (name == "recompute-frame") return to_int(v, &o->recompute_frame);
    if (name == "max-frames-latency") return to_int(v, &o->max_frames_latency);
    if (name == "snip-edges") return b(&o->snip_edges);
    return false;
  }
  if (name == "pitch-scale") return to_float(v, &o->pitch_scale);
  if (name == "pov-scale") return to_float(v, &o->pov_scale);
  if (name == "pov-offset") return to_float(v, &o->pov_offset);
  if (name == "delta-pitch-scale") return to_float(v, &o->delta_pitch_scale);
  if (name == "delta-pitch-noise-stddev") return to_float(v, &o->delta_pitch_noise_stddev);
  if (name == "normalization-left-context") return to_int(v, &o->normalization_left_context);
  if (name == "normalization-right-context") return to_int(v, &o->normalization_right_context);
  if (name == "delta-window") return to_int(v, &o->delta_window);
  if (name == "delay") return to_int(v, &o->delay);
  if (name == "add-pov-feature") return b(&o->add_pov_feature);
  if (name == "add-normalized-log-pitch") return b(&o->add_normalized_log_pitch);
  if (name == "add-delta-pitch") return b(&o->add_delta_pitch);
  if (name == "add-raw-log-pitch") return b(&o->add_raw_log_pitch);
  if (name == "noise-seed") {
    if (v.empty()) return false;
    char* end = nullptr;
    o->noise_seed = strtoull(v.c_str(), &end, 10);
    return !*end;
  }
  return false;
}

// `--name=value` options (names with '_' for '-' accepted, as ParseOptions does) and positional arguments
inline bool split_options(const std::vector<std::string>& argv, size_t from, std::map<std::string, std::string>* opts,
                          std::vector<std::string>* pos) {
  for (size_t i = from; i < argv.size(); ++i) {
    const std::string& a = argv[i];
    if (a.rfind("--", 0) == 0) {
      const size_t eq = a.find('=');
      std::string name = a.substr(2, eq == std::string::npos ? std::string::npos : eq - 2);
      for (char& c : name) if (c == '_') c = '-';
      (*opts)[name] = eq == std::string::npos ? "" : a.substr(eq + 1);
    } else {
      pos->push_back(a);
    }
  }
  return true;
}

// --config=<file> as the tools read it (one --x=y per line, # comments; read first, so the command line overrides it): the file's
// options in front of the others.  false: a file that cannot be read or a line that is no option
inline bool with_config(const std::vector<std::string>& argv, std::vector<std::string>* out) {
  std::vector<std::string> head, rest;
  for (size_t i = 0; i < argv.size(); ++i) {
    const std::string& a = argv[i];
    if (i > 0 && a.rfind("--config=", 0) == 0) {
      std::string path = a.substr(9);
      while (!path.empty() && isspace((unsigned char)path.back())) path.pop_back();
      while (!path.empty() && isspace((unsigned char)path.front())) path.erase(path.begin());
      std::ifstream f(path);
      if (!f) return false;
      std::string line;
      while (std::getline(f, line)) {
        line = line.substr(0, line.find('#'));
        while (!line.empty() && isspace((unsigned char)line.back())) line.pop_back();
        while (!line.empty() && isspace((unsigned char)line.front())) line.erase(line.begin());
        if (line.empty()) continue;
        if (line.rfind("--", 0) != 0) return false;
        head.push_back(line);
      }
    } else {
      rest.push_back(a);
    }
  }
  out->clear();
  if (!rest.empty()) out->push_back(rest[0]);
  out->insert(out->end(), head.begin(), head.end());
  out->insert(out->end(), rest.begin() + (rest.empty() ? 0 : 1), rest.end());
  return true;
}

// the commands of a pipe line, split at the `|` outside quotes; false when a quote is left open
inline bool split_pipe(const std::string& cmd, std::vector<std::string>* segs) {
  segs->clear();
  size_t b = 0;
  bool in_q = false;
  char q = 0;
  for (size_t i = 0; i <= cmd.size(); ++i) {
    if (i < cmd.size() && (cmd[i] == '\'' || cmd[i] == '"')) { if (!in_q) { in_q = true; q = cmd[i]; } else if (q == cmd[i]) in_q = false; }
    if (i == cmd.size() || (cmd[i] == '|' && !in_q)) { segs->push_back(cmd.substr(b, i - b)); b = i + 1; }
  }
  return !in_q;
}

// an input of paste-feats that is itself a pipe, "ark[,s,cs]:tool ... | tool ... |": the argument vectors of its commands
inline bool inner_pipe(const std::string& spec, std::vector<std::vector<std::string>>* out) {
  const size_t colon = spec.find(':');
  if (colon == std::string::npos) return false;
  std::string head = spec.substr(0, colon), cmd = spec.substr(colon + 1);
  std::vector<std::string> hs;
  for (size_t b = 0;;) { const size_t c = head.find(',', b); hs.push_back(head.substr(b, c == std::string::npos ? c : c - b)); if (c == std::string::npos) break; b = c + 1; }
  if (hs[0] != "ark") return false;
  for (size_t i = 1; i < hs.size(); ++i) if (hs[i] != "s" && hs[i] != "cs") return false;
  while (!cmd.empty() && isspace((unsigned char)cmd.back())) cmd.pop_back();
  if (cmd.empty() || cmd.back() != '|') return false;
  cmd.pop_back();
  std::vector<std::string> segs;
  if (!split_pipe(cmd, &segs)) return false;
  out->clear();
  for (const std::string& s : segs) {
    std::vector<std::string> argv;
    if (!shell_split(s, &argv) || argv.empty()) return false;
    out->push_back(argv);
  }
  return true;
}

// a wav table rspecifier without its options (scp,p:x -> scp:x); "" for anything that is not a plain table
inline std::string wav_source(std::string src) {
  while (!src.empty() && isspace((unsigned char)src.back())) src.pop_back();
  const size_t c = src.find(':');
  if (c == std::string::npos || src.empty() || src.back() == '|') return "";
  const std::string k = src.substr(0, src.find_first_of(",:"));
  if (k != "ark" && k != "scp") return "";
  std::string path = src.substr(c + 1);
  while (!path.empty() && isspace((unsigned char)path.front())) path.erase(path.begin());
  return k + ":" + path;
}

inline bool table_kind(const std::string& spec) {  // ark:... / scp:... (with options), not itself a command
  const size_t c = spec.find(':');
  if (c == std::string::npos) return false;
  const std::string k = spec.substr(0, spec.find_first_of(",:"));
  return k == "ark" || k == "scp";
}

inline bool parse_feature_pipeline(const std::string& rspecifier, Pipeline* out) {
  const size_t colon = rspecifier.find(':');
  if (colon == std::string::npos || rspecifier.substr(0, rspecifier.find_first_of(",:")) != "ark") return false;
  std::string cmd = rspecifier.substr(colon + 1);
  while (!cmd.empty() && isspace((unsigned char)cmd.back())) cmd.pop_back();
  if (cmd.empty() || cmd.back() != '|') return false;
  cmd.pop_back();
  std::vector<std::string> segs;
  if (!split_pipe(cmd, &segs)) return false;
  Pipeline p;
  for (size_t si = 0; si < segs.size(); ++si) {
    std::vector<std::string> argv, pos;
    std::map<std::string, std::string> o;
    if (!shell_split(segs[si], &argv) || argv.empty()) return false;
    std::string tool = argv[0];
    if (tool.find('/') != std::string::npos) tool = tool.substr(tool.rfind('/') + 1);
    split_options(argv, 1, &o, &pos);
    auto only = [&](std::initializer_list<const char*> names) {
      for (const auto& kv : o) { bool ok = false; for (const char* n : names) ok = ok || kv.first == n; if (!ok) return false; }
      return true;
    };
    if (si == 0 && tool == "paste-feats") {               // featbin/paste-feats.cc over the two extractors: the pipe starts at the audio
      if (!only({"length-tolerance"}) || pos.size() != 3 || pos[2] != "ark:-") return false;
      if (o.count("length-tolerance") && (!to_int(o["length-tolerance"], &p.tolerance) || p.tolerance < 0)) return false;
      std::vector<std::vector<std::string>> fb, pt;
      if (!inner_pipe(pos[0], &fb) || !inner_pipe(pos[1], &pt) || fb.size() != 1 || pt.size() != 2) return false;
      const char* tools[3] = {"compute-fbank-feats", "compute-kaldi-pitch-feats", "process-kaldi-pitch-feats"};
      std::vector<std::string> args[3];
      std::map<std::string, std::string> io[3];
      std::vector<std::string> ipos[3];
      for (int k = 0; k < 3; ++k) {
        const std::vector<std::string>& av = k == 0 ? fb[0] : pt[k - 1];
        std::string t = av[0];
        if (t.find('/') != std::string::npos) t = t.substr(t.rfind('/') + 1);
        if (t != tools[k] || !with_config(av, &args[k])) return false;
        split_options(args[k], 1, &io[k], &ipos[k]);
      }
      if (ipos[0].size() != 2 || ipos[0][1] != "ark:-" || ipos[1].size() != 2 || ipos[1][1] != "ark:-") return false;
      if (ipos[2].size() != 2 || ipos[2][0] != "ark:-" || ipos[2][1] != "ark:-") return false;
      int verbose = 0;
      eesen_fbank_opts_default(&p.fbank);
      for (const auto& kv : io[0]) {
        if (kv.first == "channel") { if (!to_int(kv.second, &p.wave.channel)) return false; }
        else if (kv.first == "min-duration") { if (!to_float(kv.second, &p.wave.min_duration)) return false; }
        else if (kv.first == "output-format") { if (kv.second != "kaldi") return false; }
        else if (kv.first == "verbose") { if (!to_int(kv.second, &verbose)) return false; }
        else if (!set_fbank_option(kv.first, kv.second, &p.fbank)) return false;
      }
      if (!p.fbank.round_to_power_of_two) return false;
      eesen_pitch_opts_default(&p.pitch);
      for (int k = 1; k < 3; ++k)
        for (const auto& kv : io[k]) {
          if (kv.first == "verbose" || (k == 2 && kv.first == "srand")) { if (!to_int(kv.second, &verbose)) return false; }
          else if (!set_pitch_option(k - 1, kv.first, kv.second, &p.pitch)) return false;
        }
      // what the device extractor refuses (eesen_pitch_create) stays with the reference's tool
      if (p.pitch.preemph_coeff != 0.f || p.pitch.frames_per_chunk != 0 || p.pitch.simulate_first_pass_online || p.pitch.nccf_ballast_online) return false;
      const std::string src = wav_source(ipos[0][0]);
      if (src.empty() || src != wav_source(ipos[1][0])) return false;
      p.source = ipos[0][0];
      p.has_fbank = p.has_pitch = true;
      p.wave.samp_freq = p.fbank.samp_freq;
      p.stages.push_back({EESEN_FEAT_FBANK_PITCH, p.tolerance, 0});
      continue;
    }
    if (si == 0 && tool == "compute-fbank-feats") {       // featbin/compute-fbank-feats.cc: the pipe starts at the audio
      if (pos.size() != 2 || pos[1] != "ark:-") return false;
      eesen_fbank_opts_default(&p.fbank);
      for (const auto& kv : o) {
        if (kv.first == "channel") { if (!to_int(kv.second, &p.wave.channel)) return false; }
        else if (kv.first == "min-duration") { if (!to_float(kv.second, &p.wave.min_duration)) return false; }
        else if (kv.first == "output-format") { if (kv.second != "kaldi") return false; }
        else if (!set_fbank_option(kv.first, kv.second, &p.fbank)) return false;
      }
      if (!p.fbank.round_to_power_of_two) return false;
      std::string src = pos[0];
      while (!src.empty() && isspace((unsigned char)src.back())) src.pop_back();
      if (!table_kind(src) || src.back() == '|') return false;
      p.source = pos[0];
      p.has_fbank = true;
      p.wave.samp_freq = p.fbank.samp_freq;
      p.stages.push_back({EESEN_FEAT_FBANK, 0, 0});
      continue;
    }
    if (si == 1 && p.has_fbank && tool == "apply-cmvn") {  // reads the head's output: ark:-
      if (!only({"utt2spk", "norm-vars", "norm-means"}) || pos.size() != 3 || pos[1] != "ark:-" || pos[2] != "ark:-") return false;
      bool norm_means = true, norm_vars = false;
      if (o.count("norm-means") && !to_bool(o["norm-means"], &norm_means)) return false;
      if (o.count("norm-vars") && !to_bool(o["norm-vars"], &norm_vars)) return false;
      if (norm_vars && !norm_means) return false;
      if (norm_means) {
        p.cmvn = pos[0];
        p.utt2spk = o.count("utt2spk") ? o["utt2spk"] : "";
        p.norm_vars = norm_vars;
        p.stages.push_back({EESEN_FEAT_CMVN, norm_vars ? 1 : 0, 0});
      }
      continue;
    }
    if (si == 0) {
      if (tool == "apply-cmvn") {                         // featbin/apply-cmvn.cc:36-47
        if (!only({"utt2spk", "norm-vars", "norm-means"}) || pos.size() != 3 || pos[2] != "ark:-") return false;
        bool norm_means = true, norm_vars = false;
        if (o.count("norm-means") && !to_bool(o["norm-means"], &norm_means)) return false;
        if (o.count("norm-vars") && !to_bool(o["norm-vars"], &norm_vars)) return false;
        if (norm_vars && !norm_means) return false;       // the tool itself refuses this (:55-56): let it say so
        p.source = pos[1];
        if (norm_means) {
          p.cmvn = pos[0];
          p.utt2spk = o.count("utt2spk") ? o["utt2spk"] : "";
          p.norm_vars = norm_vars;
          p.stages.push_back({EESEN_FEAT_CMVN, norm_vars ? 1 : 0, 0});
        }
      } else if (tool == "copy-feats") {
        if (!o.empty() || pos.size() != 2 || pos[1] != "ark:-") return false;
        p.source = pos[0];
      } else {
        return false;
      }
      std::string src = p.source;
      while (!src.empty() && isspace((unsigned char)src.back())) src.pop_back();
      if (!table_kind(src) || src.back() == '|') return false;
      continue;
    }
    if (pos.size() != 2 || pos[0] != "ark:-" || pos[1] != "ark:-") return false;
    if (tool == "splice-feats") {                          // featbin/splice-feats.cc:36-40: both contexts default to 4
      int L = 4, R = 4;
      if (!only({"left-context", "right-context"})) return false;
      if (o.count("left-context") && !to_int(o["left-context"], &L)) return false;
      if (o.count("right-context") && !to_int(o["right-context"], &R)) return false;
      if (L < 0 || R < 0) return false;
      p.stages.push_back({EESEN_FEAT_SPLICE, L, R});
    } else if (tool == "subsample-feats") {                // featbin/subsample-feats.cc:46-55
      int n = 1, off = 0;
      if (!only({"n", "offset"})) return false;
      if (o.count("n") && !to_int(o["n"], &n)) return false;
      if (o.count("offset") && !to_int(o["offset"], &off)) return false;
      if (n == 0 || off < 0 || (n < 0 && off != 0)) return false;
      p.stages.push_back({EESEN_FEAT_SUBSAMPLE, n, off});
    } else if (tool == "add-deltas") {                     // featbin/add-deltas.cc:33-38; DeltaFeaturesOptions: order 2, window 2
      int order = 2, window = 2, truncate = 0;
      if (!only({"delta-order", "delta-window", "truncate"})) return false;
      if (o.count("delta-order") && !to_int(o["delta-order"], &order)) return false;
      if (o.count("delta-window") && !to_int(o["delta-window"], &window)) return false;
      if (o.count("truncate") && !to_int(o["truncate"], &truncate)) return false;
      if (truncate != 0 || order < 0 || order > 8 || window <= 0 || window > 16) return false;
      p.stages.push_back({EESEN_FEAT_DELTAS, order, window});
    } else {
      return false;
    }
  }
  *out = p;
  return true;
}

// Matrix<double>::Read (src/cpucompute/matrix.cc:1012-1100): DM, or FM converted, or text.  CMVN statistics are doubles.
struct Mat64 { std::vector<double> v; int rows = 0, cols = 0; };
inline Mat64 read_matrix64(std::istream& is) {
  Mat64 m;
  if (is.peek() == '\0') {
    is.get(); is.get();
    std::string tok;
    is >> tok;
    is.get();
    if (tok != "DM" && tok != "FM") throw std::runtime_error("expected DM or FM, got " + tok);
    m.rows = read_sized_int(is); m.cols = read_sized_int(is);
    m.v.resize((size_t)m.rows * m.cols);
    if (tok == "DM") {
      is.read(reinterpret_cast<char*>(m.v.data()), m.v.size() * 8);
    } else {
      std::vector<float> f(m.v.size());
      is.read(reinterpret_cast<char*>(f.data()), f.size() * 4);
      for (size_t i = 0; i < f.size(); ++i) m.v[i] = f[i];
    }
    need(is, "matrix data");
    return m;
  }
  char c;
  do { need(is.get(c), "text matrix"); } while (c != '[');
  std::string body;
  std::getline(is, body, ']');
  std::istringstream rows(body);
  std::string line;
  while (std::getline(rows, line)) {
    std::istringstream ls(line);
    double f;
    int n = 0;
    while (ls >> f) { m.v.push_back(f); ++n; }
    if (n) { if (m.cols && n != m.cols) throw std::runtime_error("ragged text matrix"); m.cols = n; ++m.rows; }
  }
  std::getline(is, line);
  return m;
}

// RandomAccessDoubleMatrixReaderMapped(cmvn_rspecifier, utt2spk_rspecifier) of apply-cmvn.cc:80-81, or the single matrix of its
// rxfilename form (:115-122).  The normaliser ([2 x dim] floats: offsets, scales) is computed once per speaker by the library's
// eesen_cmvn_norm (ApplyCmvn's own arithmetic, src/feat/cmvn.cc:78-108).
class CmvnTable {
 public:
  CmvnTable(const std::string& spec, const std::string& utt2spk, bool norm_vars) : norm_vars_(norm_vars) {
    if (table_kind(spec)) {
      const Spec sp = parse_spec(spec);
      InStream in(sp.path);
      std::istream& f = in.get();
      if (sp.kind == "ark") {
        for (std::string key = read_key(f); !key.empty(); key = read_key(f)) stats_[key] = read_matrix64(f);
      } else {
        std::string line;
        while (std::getline(f, line)) {
          std::istringstream ls(line);
          std::string key, loc;
          if (!(ls >> key >> loc)) continue;
          std::streamoff off = 0;
          const size_t c = loc.rfind(':');
          if (c != std::string::npos && c + 1 < loc.size() && loc.find_first_not_of("0123456789", c + 1) == std::string::npos) {
            off = std::stoll(loc.substr(c + 1));
            loc = loc.substr(0, c);
          }
          std::ifstream a(loc, std::ios::binary);
          if (!a) throw std::runtime_error("cannot open " + loc);
          a.seekg(off);
          stats_[key] = read_matrix64(a);
        }
      }
      if (!utt2spk.empty()) {
        const Spec us = parse_spec(utt2spk);
        if (us.kind != "ark") throw std::runtime_error("utt2spk: only ark: tables are supported");
        InStream uin(us.path);
        std::string line;
        while (std::getline(uin.get(), line)) {
          std::istringstream ls(line);
          std::string u, s;
          if (ls >> u >> s) map_[u] = s;
        }
        mapped_ = true;
      }
    } else {
      if (!utt2spk.empty()) throw std::runtime_error("--utt2spk option not compatible with rxfilename as input (did you forget ark:?)");
      std::string loc = spec;
      std::streamoff off = 0;
      const size_t c = loc.rfind(':');
      if (loc.find('|') == std::string::npos && c != std::string::npos && c + 1 < loc.size() &&
          loc.find_first_not_of("0123456789", c + 1) == std::string::npos) {
        off = std::stoll(loc.substr(c + 1));
        loc = loc.substr(0, c);
      }
      InStream in(loc);
      if (off) in.get().seekg(off);
      global_ = norm(read_matrix64(in.get()));
      is_global_ = true;
    }
  }
  // nullptr: no statistics for this utterance (apply-cmvn then writes nothing for it, :87-92)
  const std::vector<float>* lookup(const std::string& utt) {
    if (is_global_) return &global_;
    std::string key = utt;
    if (mapped_) {
      auto m = map_.find(utt);
      if (m == map_.end()) return nullptr;
      key = m->second;
    }
    auto c = cache_.find(key);
    if (c != cache_.end()) return &c->second;
    auto s = stats_.find(key);
    if (s == stats_.end()) return nullptr;
    return &(cache_[key] = norm(s->second));
  }
  static int dim(const std::vector<float>& n) { return (int)n.size() / 2; }

 private:
  std::vector<float> norm(const Mat64& m) const {
    std::vector<float> out((size_t)2 * std::max(m.cols - 1, 0));
    if (eesen_cmvn_norm(m.v.data(), m.rows, m.cols, norm_vars_ ? 1 : 0, out.data()) != EESEN_OK) throw std::runtime_error(eesen_last_error());
    return out;
  }
  bool norm_vars_, mapped_ = false, is_global_ = false;
  std::map<std::string, Mat64> stats_;
  std::map<std::string, std::string> map_;
  std::map<std::string, std::vector<float>> cache_;
  std::vector<float> global_;
};

}  // namespace ktab
