// ctc_decode.cc -- lexicon-free CTC prefix beam search of utterances, over the C-ABI of include/eesen_hip.h, host C++ only.  The
// reference has no such binary: it decodes ONE utterance per process through a TLG graph and its WFST decoder over
// net-output-extract's output.  Here, per group of --num-sequence utterances: Net::Feedforward as net-output-extract does it ->
// optional ClassPrior::SubtractOnLogpost (the options of net-output-extract) -> eesen_ctc_decode_parallel.  Written: one int32 vector
// per hypothesis, the labels (blank-free); with --nbest > 1 under the keys utt-1, utt-2, ... (as lattice-to-nbest names them).
// With --lm a token n-gram LM (an ARPA file over the net's tokens) is fused into the search: eesen_ctc_decode_parallel_lm.
// With --lexicon the labellings are held to lexicon words separated by --space-unit, scored by an optional word n-gram LM
// (--word-lm): eesen_ctc_decode_parallel_lex; the word ids go to --words-wspecifier and word errors are counted against
// --word-ref-rspecifier.  With --word-boundary=none the lexicon has no boundary unit (the phoneme systems: nothing but CTC's blank
// between words, homophones allowed): eesen_ctc_decode_parallel_words; the word ends go to --word-ends-wspecifier.
// With --ctm-out the best hypothesis of every utterance is aligned to the frames (eesen_ctc_decode_stamps) and written as CTM lines
// `key 1 start duration word [confidence]`, the file sclite scores.
// With --rescore=true every returned hypothesis gets its exact acoustic score and the list is ranked again, optionally with a second
// LM (--rescore-lm): eesen_ctc_decode_rescore.  Everything is then written in the new order and speaks of the new best hypothesis.
// With --mbr=true every list is ranked by expected errors under its own posterior (over the second pass's totals with --rescore):
// eesen_ctc_decode_mbr.  Everything is written in that order, the errors against the references come back with it, and the summary
// adds the errors of the N-best oracle.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>

#include <unistd.h>

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
// the class id of --space-unit: a symbol of the units table, or a decimal id without one
int space_class(const std::string& unit, const std::string& units_path) {
  if (units_path.empty()) {
    if (unit.empty() || unit.find_first_not_of("0123456789") != std::string::npos || unit.size() > 9)
      throw std::runtime_error("--space-unit=" + unit + " is no decimal class id (give --lexicon-units to name it by its symbol)");
    return std::stoi(unit);
  }
  std::ifstream in(units_path);
  if (!in) throw std::runtime_error("cannot open " + units_path);
  std::string line, sym, id;
  while (std::getline(in, line)) {
    std::istringstream f(line);
    if (f >> sym >> id && sym == unit && id.find_first_not_of("0123456789") == std::string::npos && id.size() <= 9) return std::stoi(id);
  }
  throw std::runtime_error("--space-unit=" + unit + " is not in " + units_path);
}
// `symbol id` lines -> id -> symbol (the first symbol of an id wins)
std::map<int, std::string> id_symbols(const std::string& path) {
  std::ifstream in(path);
  if (!in) throw std::runtime_error("cannot open " + path);
  std::map<int, std::string> out;
  std::string line, sym, id;
  while (std::getline(in, line)) {
    std::istringstream f(line);
    if (f >> sym >> id && id.find_first_not_of("0123456789") == std::string::npos && id.size() <= 9) out.emplace(std::stoi(id), sym);
  }
  return out;
}
std::string fixed(double v, int precision) {
  char buf[512];
  snprintf(buf, sizeof buf, "%.*f", precision, v);
  return buf;
}
// the value of a --rescore-* option that is kept as text so that "not given" can stand for the first pass's value
float number_option(const std::string& name, const std::string& text) {
  char* end = nullptr;
  const double v = std::strtod(text.c_str(), &end);
  if (end == text.c_str()) throw std::runtime_error("Invalid floating-point option \"" + text + "\" of --" + name);
  return (float)v;
}
double double_option(const std::string& name, const std::string& text) {
  char* end = nullptr;
  const double v = std::strtod(text.c_str(), &end);
  if (end == text.c_str()) throw std::runtime_error("Invalid floating-point option \"" + text + "\" of --" + name);
  return v;
}
bool bool_option(const std::string& name, std::string text) {
  std::transform(text.begin(), text.end(), text.begin(), [](unsigned char c) { return (char)std::tolower(c); });
  if (text == "true" || text == "t" || text == "1") return true;
  if (text == "false" || text == "f" || text == "0") return false;
  throw std::runtime_error("Invalid format for boolean argument [expected true or false] of --" + name + ": " + text);
}
std::string fmt9(double v) {
  std::ostringstream o;
  o.precision(9);
  o << v;
  return o.str();
}
}  // namespace

int main(int argc, char** argv) {
  try {
    std::string class_frame_counts, scores_out, ref_rspecifier, lm_arpa, lm_units;
    std::string lexicon, lexicon_units, space_unit = "<SPACE>", word_lm, words_wspecifier, words_table_out, word_ref_rspecifier;
    std::string word_boundary = "unit", word_ends_wspecifier, ctm_out, ctm_units;
    double frame_shift = 0.01, conf_scale = 1.0;
    int ctm_precision = 2;
    bool ctm_conf = false;
    float prior_scale = 1.f, lm_weight = 1.f, insertion_bonus = 0.f, word_bonus = 0.f;
    bool lm_eos = false, lm_skip_oov = false, lm_lookahead = false;
    bool rescore = false;
    std::string rescore_lm, rescore_lm_weight, rescore_bonus, rescore_lm_eos;
    bool mbr = false, mbr_units = false;
    std::string mbr_scale;
    double prior_cutoff = 1e-10, blank_scale = 1.0, frame_limit = 1e5;
    int num_sequence = 1, device = 0, beam = 16, max_classes = 20, nbest = 1;
    std::string use_gpu = "yes";
    eesen_tools::ParseOptions po(
        "Decode utterances without a lexicon: CTC prefix beam search over the network's outputs.\n"
        "Writes the most probable label sequences (blank-free int32 vectors); with --nbest > 1 under the keys utt-1, utt-2, ...\n"
        "\n"
        "Usage:  ctc-decode [options] <model-in> <feature-rspecifier> <hyp-wspecifier>\n"
        "e.g.: \n"
        "ctc-decode --beam=16 net ark:features.ark ark:hyp.ark\n");
    po.Register("class-frame-counts", &class_frame_counts, "Vector with frame-counts of classes to compute log-priors; the search then runs on "
                                                           "log-posteriors minus the scaled log-priors");
    po.Register("prior-scale", &prior_scale, "Scaling factor to be applied on class-log-priors");
    po.Register("prior-cutoff", &prior_cutoff, "Classes with priors lower than cutoff will have 0 likelihood");
    po.Register("blank-scale", &blank_scale, "Scale probability of class 0 (blank) by this factor");
    po.Register("beam", &beam, "Prefixes kept per frame (1 .. 64)");
    po.Register("max-classes", &max_classes, "Non-blank classes a prefix is extended by per frame: the best of the frame (1 .. 64; beam * max-classes <= 2048)");
    po.Register("nbest", &nbest, "Hypotheses written per utterance (1 .. beam)");
    po.Register("scores-out", &scores_out, "Also write `key log-probability` text lines, one per hypothesis, to this file");
    po.Register("ref-rspecifier", &ref_rspecifier, "Reference label sequences: the token errors of the best hypotheses against them are counted");
    po.Register("lm", &lm_arpa, "ARPA file of a token n-gram LM (its words: the symbols of --lm-units, or class ids) fused into the search");
    po.Register("lm-units", &lm_units, "units.txt of the LM's words: `symbol id` per line; without it the ARPA's words are decimal class ids");
    po.Register("lm-weight", &lm_weight, "Weight of the LM's log-probability of every label");
    po.Register("insertion-bonus", &insertion_bonus, "Added per label, in nats");
    po.Register("lm-eos", &lm_eos, "Add the weighted log-probability of </s> at the end of every hypothesis");
    po.Register("lexicon", &lexicon, "Lexicon, `word unit unit ...` per spelling: the hypotheses are its words separated by --space-unit");
    po.Register("lexicon-units", &lexicon_units, "units.txt of the lexicon's units: `symbol id` per line; without it they are decimal class ids");
    po.Register("space-unit", &space_unit, "The unit between words: a symbol of --lexicon-units, or a decimal class id without it");
    po.Register("word-boundary", &word_boundary, "unit: words are separated by --space-unit; none: nothing but CTC's blank stands between words and "
                                                 "several words may share a spelling (the phoneme systems)");
    po.Register("word-ends-wspecifier", &word_ends_wspecifier, "With --word-boundary=none: also write, per hypothesis, the number of labels up to and "
                                                               "including each word's last (int32 vectors)");
    po.Register("word-lm", &word_lm, "ARPA file of a word n-gram LM over the lexicon's words, stepped once per word (weight: --lm-weight)");
    po.Register("word-bonus", &word_bonus, "Added per word, in nats");
    po.Register("lm-skip-oov", &lm_skip_oov, "Drop the n-grams of --word-lm that hold a word outside the lexicon instead of refusing the file");
    po.Register("lm-lookahead", &lm_lookahead, "Rank the candidates of a frame as if the most probable word (by --word-lm's unigrams) that the "
                                               "lexicon still allows had been paid already: a narrow --beam prunes better");
    po.Register("words-wspecifier", &words_wspecifier, "Also write the word ids of every hypothesis (int32 vectors, the keys of <hyp-wspecifier>)");
    po.Register("words-table-out", &words_table_out, "Write the lexicon's `word id` table to this file");
    po.Register("word-ref-rspecifier", &word_ref_rspecifier, "Reference word-id sequences: the word errors of the best hypotheses against them are counted");
    po.Register("ctm-out", &ctm_out, "Also write the best hypothesis of every utterance as CTM lines `key 1 start duration word` to this file: "
                                     "its words aligned to the frames");
    po.Register("frame-shift", &frame_shift, "Seconds per frame of the network's output (the recipes subsample by 3: 0.03)");
    po.Register("ctm-precision", &ctm_precision, "Digits behind the point of the CTM's times and confidences");
    po.Register("ctm-conf", &ctm_conf, "A sixth CTM column: the word's posterior over the --nbest hypotheses");
    po.Register("conf-scale", &conf_scale, "Scale of the hypotheses' log-probabilities in that posterior (>= 0)");
    po.Register("ctm-units", &ctm_units, "units.txt naming the CTM's words without a lexicon: `symbol id` per line (default: --lm-units; else class ids)");
    po.Register("rescore", &rescore, "Second pass: score every hypothesis exactly, rank the list again and write everything in the new order");
    po.Register("rescore-lm", &rescore_lm, "ARPA file of the second pass's LM: over --lm-units' tokens, or over the lexicon's words with --lexicon "
                                           "(default: the first pass's LM scores)");
    po.Register("rescore-lm-weight", &rescore_lm_weight, "Weight of the LM score in the second pass (default: --lm-weight)");
    po.Register("rescore-bonus", &rescore_bonus, "Added per label or, with --lexicon, per word in the second pass (default: --insertion-bonus or --word-bonus)");
    po.Register("rescore-lm-eos", &rescore_lm_eos, "true|false: --rescore-lm's log-probability of </s> joins at the end (default: --lm-eos)");
    po.Register("mbr", &mbr, "Minimum Bayes risk: rank every list by its hypotheses' expected errors under the list's own posterior and write "
                             "everything in that order");
    po.Register("mbr-scale", &mbr_scale, "Scale of the hypotheses' log-probabilities in that posterior, >= 0 (default: 1.0)");
    po.Register("mbr-units", &mbr_units, "Count the expected errors in labels even with --lexicon (default: in labels, or in words with --lexicon)");
    po.Register("use-gpu", &use_gpu, "yes|no|optional (accepted for the recipes' command lines; this tool always runs on the GPU)");
    po.Register("num-sequence", &num_sequence, "Utterances forwarded and decoded together");
    po.Register("frame-limit", &frame_limit, "Max number of frames forwarded together");
    po.Register("device", &device, "GPU index");
    po.Read(argc, argv);
    std::vector<std::string> args;
    for (int i = 1; i <= po.NumArgs(); ++i) args.push_back(po.GetArg(i));
    if (args.size() != 3) {
      po.PrintUsage();
      return 1;
    }
    if (!rescore && !(rescore_lm.empty() && rescore_lm_weight.empty() && rescore_bonus.empty() && rescore_lm_eos.empty()))
      throw std::runtime_error("--rescore-lm, --rescore-lm-weight, --rescore-bonus and --rescore-lm-eos need --rescore=true");
    if (!mbr && (!mbr_scale.empty() || mbr_units)) throw std::runtime_error("--mbr-scale and --mbr-units need --mbr=true");
    const double mbr_c = mbr_scale.empty() ? 1.0 : double_option("mbr-scale", mbr_scale);
    const float second_weight = rescore_lm_weight.empty() ? lm_weight : number_option("rescore-lm-weight", rescore_lm_weight);
    const float second_bonus = rescore_bonus.empty() ? (lexicon.empty() ? insertion_bonus : word_bonus) : number_option("rescore-bonus", rescore_bonus);
    const bool second_eos = rescore_lm_eos.empty() ? lm_eos : bool_option("rescore-lm-eos", rescore_lm_eos);
    eesen_net_t* net = nullptr;
    eesen_feeder_t* feeder = nullptr;
    eesen_ctc_t* ctc = nullptr;
    ck(eesen_net_create(device, nullptr, &net));
    ck(eesen_net_read(net, args[0].c_str()));
    ck(eesen_net_set_train_mode(net, 0));
    ck(eesen_feeder_create(device, nullptr, 1, &feeder));
    ck(eesen_ctc_create(device, nullptr, &ctc));
    ck(eesen_ctc_set_guard(ctc, net));       // hypotheses of a timed-out forward pass come back as NaN, never as table entries
    int D = 0, K = 0;
    ck(eesen_net_input_dim(net, &D));
    ck(eesen_net_output_dim(net, &K));
    eesen_lm_t* lm = nullptr;
    if (!lexicon.empty() && !lm_arpa.empty()) throw std::runtime_error("--lexicon together with --lm: the token LM and the word LM cannot be combined");
    if (!lm_arpa.empty()) ck(eesen_lm_create_from_arpa(lm_arpa.c_str(), lm_units.empty() ? nullptr : lm_units.c_str(), K, &lm));
    else if (!lm_units.empty() && rescore_lm.empty()) throw std::runtime_error("--lm-units without --lm");
    eesen_lm_t* second_lm = nullptr;
    eesen_lex_t* lex = nullptr;
    int V = 0;
    if (word_boundary != "unit" && word_boundary != "none") throw std::runtime_error("--word-boundary=" + word_boundary + " is neither unit nor none");
    const bool unspaced = word_boundary == "none";
    if (unspaced && lexicon.empty()) throw std::runtime_error("--word-boundary=none needs --lexicon");
    if (unspaced && space_unit != "<SPACE>") throw std::runtime_error("--space-unit=" + space_unit + " together with --word-boundary=none: there is no unit between words");
    if (!unspaced && !word_ends_wspecifier.empty()) throw std::runtime_error("--word-ends-wspecifier needs --word-boundary=none");
    if (!lexicon.empty()) {
      if (unspaced) {
        ck(eesen_lex_create_unspaced(lexicon.c_str(), lexicon_units.empty() ? nullptr : lexicon_units.c_str(), K, &lex));
        int H = 0;
        ck(eesen_lex_max_homophones(lex, &H));
        std::cerr << "LOG (ctc-decode:main()) the largest homophone set of " << lexicon << " holds " << H << " words" << std::endl;
      } else {
        ck(eesen_lex_create(lexicon.c_str(), lexicon_units.empty() ? nullptr : lexicon_units.c_str(), K, space_class(space_unit, lexicon_units), &lex));
      }
      ck(eesen_lex_info(lex, &V, nullptr, nullptr));
      if (!words_table_out.empty()) ck(eesen_lex_write_words(lex, words_table_out.c_str()));
      // a word LM reads its words through the lexicon's table
      auto word_lm_of = [&](const std::string& arpa, eesen_lm_t** made) {
        std::string table = words_table_out;
        if (table.empty()) {   // a file of our own, created exclusively (mkstemp), gone as soon as the LM has read it
          const char* tmpdir = getenv("TMPDIR");
          table = std::string(tmpdir && tmpdir[0] ? tmpdir : "/tmp") + "/ctc-decode-words.XXXXXX";
          const int fd = mkstemp(&table[0]);
          if (fd < 0) throw std::runtime_error("cannot create a temporary file for the words table: " + table);
          close(fd);
        }
        int rc = words_table_out.empty() ? eesen_lex_write_words(lex, table.c_str()) : EESEN_OK;
        if (rc == EESEN_OK) rc = eesen_lm_create_from_arpa_ex(arpa.c_str(), table.c_str(), V + 1, lm_skip_oov ? 1 : 0, made);
        if (words_table_out.empty()) std::remove(table.c_str());
        ck(rc);
        long long dropped = 0;
        ck(eesen_lm_oov_dropped(*made, &dropped));
        if (lm_skip_oov) std::cerr << "LOG (ctc-decode:main()) " << dropped << " n-grams of " << arpa << " hold a word outside the lexicon and were dropped" << std::endl;
      };
      if (!word_lm.empty()) word_lm_of(word_lm, &lm);
      if (!rescore_lm.empty()) word_lm_of(rescore_lm, &second_lm);
    } else if (!lexicon_units.empty() || !word_lm.empty() || !words_wspecifier.empty() || !words_table_out.empty() || !word_ref_rspecifier.empty() ||
               word_bonus != 0.f || lm_skip_oov) {
      throw std::runtime_error("--lexicon-units, --word-lm, --word-bonus, --lm-skip-oov, --words-wspecifier, --words-table-out and --word-ref-rspecifier need --lexicon");
    }
    if (!lex && !rescore_lm.empty()) ck(eesen_lm_create_from_arpa(rescore_lm.c_str(), lm_units.empty() ? nullptr : lm_units.c_str(), K, &second_lm));
    if (lm_lookahead) {
      if (!lex) throw std::runtime_error("--lm-lookahead needs --lexicon and --word-lm");
      ck(eesen_ctc_set_lm_lookahead(ctc, 1));   // (without --word-lm the library refuses the first decode call)
      if (lm) {
        int nodes = 0;
        ck(eesen_lex_info(lex, nullptr, &nodes, nullptr));
        std::vector<float> la(nodes);
        ck(eesen_lex_lookahead(lex, lm, la.data(), nodes));
        std::cerr << "LOG (ctc-decode:main()) unigram look-ahead over " << nodes << " lexicon nodes, la in [" << fmt9(*std::min_element(la.begin(), la.end()))
                  << ", " << fmt9(la[0]) << "]" << std::endl;
      }
    }
    // the CTM's word symbols: the lexicon's words, else the units of --ctm-units / --lm-units, else decimal class ids
    std::map<int, std::string> ctm_symbols;
    std::ofstream ctm;
    long num_ctm_words = 0;
    if (!ctm_out.empty()) {
      if (ctm_precision < 0 || ctm_precision > 17) throw std::runtime_error("--ctm-precision=" + std::to_string(ctm_precision) + " is outside [0, 17]");
      if (!std::isfinite(frame_shift) || frame_shift <= 0) throw std::runtime_error("--frame-shift must be positive");
      if (lex) {
        std::string table = words_table_out;
        if (table.empty()) {
          const char* tmpdir = getenv("TMPDIR");
          table = std::string(tmpdir && tmpdir[0] ? tmpdir : "/tmp") + "/ctc-decode-words.XXXXXX";
          const int fd = mkstemp(&table[0]);
          if (fd < 0) throw std::runtime_error("cannot create a temporary file for the words table: " + table);
          close(fd);
          const int rc = eesen_lex_write_words(lex, table.c_str());
          if (rc == EESEN_OK) ctm_symbols = id_symbols(table);
          std::remove(table.c_str());
          ck(rc);
        } else {
          ctm_symbols = id_symbols(table);
        }
      } else if (!ctm_units.empty() || !lm_units.empty()) {
        ctm_symbols = id_symbols(ctm_units.empty() ? lm_units : ctm_units);
      }
      ctm.open(ctm_out);
      if (!ctm) throw std::runtime_error("cannot open " + ctm_out);
    } else if (!ctm_units.empty() || ctm_conf) {
      throw std::runtime_error("--ctm-units and --ctm-conf need --ctm-out");
    }
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
    std::map<std::string, std::vector<int32_t>> refs;
    if (!ref_rspecifier.empty()) refs = read_targets(ref_rspecifier);
    std::map<std::string, std::vector<int32_t>> word_refs;
    if (!word_ref_rspecifier.empty()) word_refs = read_targets(word_ref_rspecifier);
    std::unique_ptr<IntVectorWriter> words_writer;
    if (!words_wspecifier.empty()) words_writer.reset(new IntVectorWriter(words_wspecifier));
    std::unique_ptr<IntVectorWriter> ends_writer;
    if (!word_ends_wspecifier.empty()) ends_writer.reset(new IntVectorWriter(word_ends_wspecifier));
    FeatureReader reader(piped ? pipe.source : args[1], piped ? pipe.wave_mode() : nullptr);
    IntVectorWriter writer(args[2]);
    std::ofstream scores;
    if (!scores_out.empty()) {
      scores.open(scores_out);
      if (!scores) throw std::runtime_error("cannot open " + scores_out);
    }
    long num_done = 0, num_empty = 0, num_dead = 0, tok_err = 0, tok_ref = 0, num_scored = 0, word_err = 0, word_ref = 0, num_word_scored = 0;
    double tot_t = 0, tot_score = 0, tot_lm = 0;
    long tot_labels = 0, num_reranked = 0;
    long tok_oracle = 0, word_oracle = 0, num_mbr_moved = 0;
    std::vector<int> order3, tok_dist, word_dist, ref_off, ref_ids, second_ranks;
    std::vector<double> post3;
    std::vector<float> am2, lm2, total2;
    std::vector<int> order2, ranks, conf_len;
    std::vector<double> conf_z, conf2;
    std::vector<std::pair<std::string, Mat>> group;
    std::vector<int> out_frames;            // per utterance of the group: frames behind the pipeline
    std::vector<const float*> cmvn;
    std::vector<int> hyp, hyp_len, words, words_len, word_ends;
    std::vector<float> score, lm_score, wconf;
    std::vector<int> wstart, wend;
    auto flush = [&]() {
      const int S = (int)group.size();
      std::vector<const float*> ptr(S);
      std::vector<int> frames(out_frames), raw_frames(S);
      for (int s = 0; s < S; ++s) { ptr[s] = group[s].second.v.data(); raw_frames[s] = group[s].second.rows; }
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
      hyp.resize((size_t)S * nbest * T); hyp_len.resize((size_t)S * nbest); score.resize((size_t)S * nbest);
      if (lex && unspaced) {
        lm_score.resize((size_t)S * nbest); words.resize((size_t)S * nbest * T); words_len.resize((size_t)S * nbest); word_ends.resize((size_t)S * nbest * T);
        ck(eesen_ctc_decode_parallel_words(ctc, frames.data(), S, out, T * S, K, old, log_pri.empty() ? 0 : 1, beam, max_classes, nbest, lex, lm, lm_weight,
                                           word_bonus, lm_eos ? 1 : 0, hyp.data(), hyp_len.data(), score.data(), lm_score.data(), words.data(),
                                           words_len.data(), word_ends.data()));
      } else if (lex) {
        lm_score.resize((size_t)S * nbest); words.resize((size_t)S * nbest * T); words_len.resize((size_t)S * nbest);
        ck(eesen_ctc_decode_parallel_lex(ctc, frames.data(), S, out, T * S, K, old, log_pri.empty() ? 0 : 1, beam, max_classes, nbest, lex, lm, lm_weight,
                                         word_bonus, lm_eos ? 1 : 0, hyp.data(), hyp_len.data(), score.data(), lm_score.data(), words.data(),
                                         words_len.data()));
      } else if (lm) {
        lm_score.resize((size_t)S * nbest);
        ck(eesen_ctc_decode_parallel_lm(ctc, frames.data(), S, out, T * S, K, old, log_pri.empty() ? 0 : 1, beam, max_classes, nbest, lm, lm_weight,
                                        insertion_bonus, lm_eos ? 1 : 0, hyp.data(), hyp_len.data(), score.data(), lm_score.data()));
      } else {
        ck(eesen_ctc_decode_parallel(ctc, frames.data(), S, out, T * S, K, old, log_pri.empty() ? 0 : 1, beam, max_classes, nbest, hyp.data(),
                                     hyp_len.data(), score.data()));
      }
      if (ctm.is_open()) {
        wstart.resize((size_t)S * nbest * T); wend.resize((size_t)S * nbest * T); wconf.resize((size_t)S * nbest * T);
        ck(eesen_ctc_decode_stamps(ctc, frames.data(), S, out, T * S, K, old, log_pri.empty() ? 0 : 1, conf_scale, nullptr, nullptr, wstart.data(),
                                   wend.data(), wconf.data(), nullptr));
      }
      if (rescore) {
        am2.resize((size_t)S * nbest); lm2.resize((size_t)S * nbest); total2.resize((size_t)S * nbest); order2.resize((size_t)S * nbest);
        ck(eesen_ctc_decode_rescore(ctc, frames.data(), S, out, T * S, K, old, log_pri.empty() ? 0 : 1, second_lm, second_weight, second_bonus,
                                    second_eos ? 1 : 0, am2.data(), lm2.data(), total2.data(), order2.data()));
      }
      if (mbr) {
        // the references in the level's tokens ride along (an utterance without one: an empty reference, never read back)
        const int level = mbr_units ? 1 : 0;
        const bool words_level = lex && !mbr_units;
        auto pack = [&](const std::map<std::string, std::vector<int32_t>>& table) {
          ref_off.assign(1, 0); ref_ids.clear();
          for (int s = 0; s < S; ++s) {
            const auto r = table.find(group[s].first);
            if (r != table.end()) ref_ids.insert(ref_ids.end(), r->second.begin(), r->second.end());
            ref_off.push_back((int)ref_ids.size());
          }
          ref_ids.push_back(0);
        };
        order3.resize((size_t)S * nbest); post3.resize((size_t)S * nbest);
        tok_dist.assign((size_t)S * nbest, -1); word_dist.assign((size_t)S * nbest, -1);
        pack(words_level ? word_refs : refs);
        ck(eesen_ctc_decode_mbr(ctc, S, level, mbr_c, rescore ? total2.data() : nullptr, ref_off.data(), ref_ids.data(), nullptr,
                                (words_level ? word_dist : tok_dist).data(), post3.data(), nullptr, order3.data()));
        if (lex && !(words_level ? refs : word_refs).empty()) {   // the other kind of reference: distances alone, at the other level
          pack(words_level ? refs : word_refs);
          ck(eesen_ctc_decode_mbr(ctc, S, 1 - level, mbr_c, rescore ? total2.data() : nullptr, ref_off.data(), ref_ids.data(), nullptr,
                                  (words_level ? tok_dist : word_dist).data(), nullptr, nullptr, nullptr));
        }
      }
      for (int s = 0; s < S; ++s) {
        const std::string& utt = group[s].first;
        const size_t e0 = (size_t)s * nbest;
        if (std::isnan(score[e0]) || (rescore && std::isnan(total2[e0])) || (mbr && std::isnan(post3[e0])))
          throw std::runtime_error("the forward pass of " + utt + " timed out on the device: no hypotheses");
        if (hyp_len[e0] < 0) {
          std::cerr << "WARNING (ctc-decode:main()) " << utt << (lex ? ", no surviving prefix ends a lexicon word on " : ", every prefix has probability zero on ")
                    << frames[s] << " frames, producing no output for this utterance" << std::endl;
          ++num_dead;
          continue;
        }
        // the first-pass ranks of the returned entries in the order they are written: by expected errors, the second pass's, or the beam's
        ranks.clear(); second_ranks.clear();
        for (int i = 0; i < nbest; ++i) {
          const int r = rescore ? order2[e0 + i] : i;
          if (r >= 0 && r < nbest && hyp_len[e0 + r] >= 0) second_ranks.push_back(r);
          const int q = mbr ? order3[e0 + i] : r;
          if (q >= 0 && q < nbest && hyp_len[e0 + q] >= 0) ranks.push_back(q);
        }
        for (size_t i = 0; i < second_ranks.size(); ++i)
          if (second_ranks[i] != (int)i) { ++num_reranked; break; }
        if (mbr && ranks[0] != second_ranks[0]) ++num_mbr_moved;
        for (size_t i = 0; i < ranks.size(); ++i) {
          const size_t e = e0 + ranks[i];
          const std::string key = nbest > 1 ? utt + "-" + std::to_string(i + 1) : utt;
          writer.Write(key, hyp.data() + e * T, hyp_len[e]);
          if (words_writer) words_writer->Write(key, words.data() + e * T, words_len[e]);
          if (ends_writer) ends_writer->Write(key, word_ends.data() + e * T, words_len[e]);
          if (scores.is_open()) {
            if (rescore) {
              scores << key << ' ' << fmt9(total2[e]) << ' ' << fmt9(am2[e]) << ' ' << fmt9(lm2[e]);
            } else {
              scores << key << ' ' << fmt9(score[e]);
              if (lm) scores << ' ' << fmt9(lm_score[e]);
            }
            scores << '\n';
          }
        }
        const size_t eb = e0 + ranks[0];   // the best hypothesis: what is scored against the references and written to the CTM
        const auto ref = refs.find(utt);
        // with --mbr the distances came back with the list (an entry that does not count has none: the host routine); the oracle is
        // the list's best
        auto oracle_of = [&](const std::vector<int>& dist, int err) {
          int best = -1;
          for (int r : ranks)
            if (dist[e0 + r] >= 0 && (best < 0 || dist[e0 + r] < best)) best = dist[e0 + r];
          return best < 0 ? err : best;
        };
        if (ref != refs.end()) {
          int err = mbr ? tok_dist[eb] : -1;
          if (err < 0) ck(eesen_edit_distance(ref->second.data(), (int)ref->second.size(), hyp.data() + eb * T, hyp_len[eb], &err));
          tok_err += err; tok_ref += (long)ref->second.size(); ++num_scored;
          if (mbr) tok_oracle += oracle_of(tok_dist, err);
        }
        const auto wref = word_refs.find(utt);
        if (wref != word_refs.end()) {
          int err = mbr ? word_dist[eb] : -1;
          if (err < 0) ck(eesen_edit_distance(wref->second.data(), (int)wref->second.size(), words.data() + eb * T, words_len[eb], &err));
          word_err += err; word_ref += (long)wref->second.size(); ++num_word_scored;
          if (mbr) word_oracle += oracle_of(word_dist, err);
        }
        if (ctm.is_open()) {   // the best hypothesis' words: a label each without a lexicon
          if (std::isnan(wconf[e0 * T])) throw std::runtime_error("the forward pass of " + utt + " timed out on the device: no time stamps");
          const int nw = lex ? words_len[eb] : hyp_len[eb];
          const int* ids = (lex ? words.data() : hyp.data()) + eb * T;
          if (rescore && ctm_conf) {   // the posterior over the list by the second pass's totals (the stamps' own is by the beam's)
            conf_z.assign(nbest, 0.0); conf_len.assign(nbest, -1); conf2.assign((size_t)nbest * T, 0.0);
            for (int r = 0; r < nbest; ++r) {
              conf_z[r] = total2[e0 + r];
              conf_len[r] = hyp_len[e0 + r] < 0 ? -1 : lex ? words_len[e0 + r] : hyp_len[e0 + r];
            }
            ck(eesen_word_confidence(nbest, conf_z.data(), conf_len.data(), (lex ? words.data() : hyp.data()) + e0 * T, wstart.data() + e0 * T,
                                     wend.data() + e0 * T, T, conf_scale, conf2.data()));
          }
          for (int j = 0; j < nw; ++j) {
            if (wstart[eb * T + j] < 0) continue;   // (a labelling too long to align)
            const auto sym = ctm_symbols.find(ids[j]);
            ctm << utt << " 1 " << fixed(frame_shift * wstart[eb * T + j], ctm_precision) << ' '
                << fixed(frame_shift * (wend[eb * T + j] - wstart[eb * T + j]), ctm_precision) << ' '
                << (sym != ctm_symbols.end() ? sym->second : std::to_string(ids[j]));
            if (ctm_conf) ctm << ' ' << fixed(rescore ? (float)conf2[(eb - e0) * T + j] : wconf[eb * T + j], ctm_precision);
            ctm << '\n';
            ++num_ctm_words;
          }
        }
        ++num_done;
        if (hyp_len[eb] == 0) ++num_empty;
        tot_t += frames[s];
        tot_score += rescore ? total2[eb] : score[eb];
        if (lm || second_lm) { tot_lm += rescore ? lm2[eb] : lm_score[eb]; tot_labels += lex ? words_len[eb] : hyp_len[eb]; }
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
          if (!n) { std::cerr << "WARNING (ctc-decode:main()) No normalization statistics available for key " << utt << ", producing no output for this utterance" << std::endl; continue; }
          if (CmvnTable::dim(*n) != pipe.cmvn_dim(m.cols))
            throw std::runtime_error("Dim mismatch in ApplyCmvn: cmvn 2x" + std::to_string(CmvnTable::dim(*n) + 1) + ", feats " + std::to_string(m.rows) + "x" + std::to_string(m.cols));
          cm = n->data();
        }
        if (m.rows == 0) { std::cerr << "WARNING (ctc-decode:main()) Empty feature matrix for key " << utt << std::endl; continue; }
        ck(eesen_feeder_pipeline_shape(feeder, m.cols, m.rows, &cols, &rows));
        if (rows == 0) { std::cerr << "WARNING (ctc-decode:main()) For utterance " << utt << ", output would have no rows, producing no output." << std::endl; continue; }
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
    if (scores.is_open()) {
      scores.close();
      if (!scores) throw std::runtime_error("write error: " + scores_out);
    }
    if (ctm.is_open()) {
      ctm.close();
      if (!ctm) throw std::runtime_error("write error: " + ctm_out);
    }
    if (!ref_rspecifier.empty()) {
      std::cerr << "LOG (ctc-decode:main()) " << tok_err << " token errors on " << tok_ref << " reference tokens of " << num_scored << " utterances" << std::endl;
      if (mbr) std::cerr << "LOG (ctc-decode:main()) " << tok_oracle << " token errors of the N-best oracle (the best of up to " << nbest << " hypotheses per utterance)" << std::endl;
      std::cerr << "LOG (ctc-decode:main()) \nTOKEN_ACCURACY >> " << 100.0 * (1.0 - (double)tok_err / (double)std::max(tok_ref, 1L)) << "% <<" << std::endl;
    }
    if (!word_ref_rspecifier.empty()) {
      std::cerr << "LOG (ctc-decode:main()) " << word_err << " word errors on " << word_ref << " reference words of " << num_word_scored << " utterances" << std::endl;
      if (mbr) std::cerr << "LOG (ctc-decode:main()) " << word_oracle << " word errors of the N-best oracle (the best of up to " << nbest << " hypotheses per utterance)" << std::endl;
      std::cerr << "LOG (ctc-decode:main()) \nWORD_ACCURACY >> " << 100.0 * (1.0 - (double)word_err / (double)std::max(word_ref, 1L)) << "% <<" << std::endl;
    }
    if (num_dead) std::cerr << "LOG (ctc-decode:main()) " << num_dead << " utterances without a hypothesis" << std::endl;
    std::cerr << "LOG (ctc-decode:main()) Done " << num_done << " utterances, " << num_empty << " empty hypotheses; average log-probability per frame "
              << (tot_t > 0 ? tot_score / tot_t : 0.0);
    if (lm || second_lm) std::cerr << "; average LM log-probability per " << (lex ? "word " : "label ") << (tot_labels > 0 ? tot_lm / tot_labels : 0.0);
    if (!ctm_out.empty()) std::cerr << "; " << num_ctm_words << " CTM words";
    if (rescore) std::cerr << "; " << num_reranked << " utterances re-ranked";
    if (mbr) std::cerr << "; " << num_mbr_moved << " utterances whose hypothesis of least expected errors is not the most probable";
    std::cerr << std::endl;
    if (second_lm) eesen_lm_destroy(second_lm);
    if (lm) eesen_lm_destroy(lm);
    if (lex) eesen_lex_destroy(lex);
    eesen_ctc_destroy(ctc);
    eesen_feeder_destroy(feeder);
    eesen_net_destroy(net);
    return num_done ? 0 : 255;
  } catch (const std::exception& e) {
    std::cerr << "ERROR (ctc-decode:main()) " << e.what() << std::endl;
    return 255;
  }
}
