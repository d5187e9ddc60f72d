// ctc_host.cpp -- host side of the Ctc object: label expansion, launch sequence, statistics, greedy
// decoding.  Replaces eesen::Ctc::EvalParallel / ErrorRateMSeq (the reference's src/net/ctc-loss.cc:101-194,
// :235-298).  The lattice arithmetic itself is in ctc.hip.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <fstream>
#include <limits>

#include "net.h"

namespace eesen {

Ctc::Ctc(int dev, void* stream) : device(dev) {
  require_device(dev);
  st = reinterpret_cast<hipStream_t>(stream);  // NULL = the device's default stream (shared with the Net)
  if (const char* e = getenv("EESEN_CTC_WAVES"); e && *e) sweep_waves = atoi(e);
}

Ctc::~Ctc() {   // drained here; the guard hook, the pinned slots and the events go with the members
  (void)hipSetDevice(device);
  (void)hipStreamSynchronize(st);
}

void Ctc::flush_pzx(PendingPzx& q) {
  if (!q.active) return;
  q.pin.wait();
  const float* pz = q.pin.as<float>();
  q.active = false;
  if (StatGuard::raised(pz, q.S * sizeof(float))) {  // computed from a timed-out forward pass (see StatGuard): not a statistic
    sequences -= q.S;
    frames -= q.nframes;
    guard.note_dropped("CTC");
    return;
  }
  double sum = 0;
  for (int s = 0; s < q.S; ++s) sum += pz[s];
  obj_sum += sum;  // ctc-loss.cc:171-177
}

void Ctc::flush() {
  EESEN_HIP_CHECK(hipSetDevice(device));
  for (unsigned k = 0; k < 2; ++k) flush_pzx(ppzx[(ppzx_idx + k) & 1]);   // oldest first
  for (unsigned k = 0; k < 2; ++k) flush_err(perr[(perr_idx + k) & 1], nullptr, nullptr);
}

void Ctc::set_profiling(int mode) {
  for (PhaseClock* c : {&clock, &align_clock, &decode_clock, &stamp_clock}) c->set_mode(mode == 2);   // (rescore_clock: always the last call's)
  mbr_accumulate = mode == 2;
  mbr_t[0] = mbr_t[1] = mbr_t[2] = 0;
}

void check_shape(const int* frame_num_utt, int S, int rows, int K, int ld, int min_K) {
  EESEN_REQUIRE(S > 0 && rows > 0 && rows % S == 0, EESEN_ERR_INVALID, "rows must be a positive multiple of the sequence count");
  if (min_K >= 2) EESEN_REQUIRE(K >= 2, EESEN_ERR_INVALID, "decoding needs the blank and at least one other class (K >= 2)");
  else if (min_K == 1) EESEN_REQUIRE(K > 0, EESEN_ERR_INVALID, "no classes");
  EESEN_REQUIRE(K > 0 && ld >= K, EESEN_ERR_INVALID, "leading dimension smaller than the class count");
  const int T = rows / S;
  for (int s = 0; s < S; ++s)
    EESEN_REQUIRE(frame_num_utt[s] >= 0 && frame_num_utt[s] <= T, EESEN_ERR_INVALID, "frame_num_utt out of range");
}

// the shape and the labels of eval_parallel, align_parallel and error_rate_mseq
static void check_batch(const int* frame_num_utt, int S, int rows, int K, int ld, const int* label_ids, const int* label_off) {
  check_shape(frame_num_utt, S, rows, K, ld, 1);
  for (int s = 0; s < S; ++s)
    EESEN_REQUIRE(label_off[s + 1] >= label_off[s], EESEN_ERR_INVALID, "label offsets must be non-decreasing");
  for (int i = label_off[0]; i < label_off[S]; ++i)
    EESEN_REQUIRE(label_ids[i] >= 0 && label_ids[i] < K, EESEN_ERR_INVALID, "label id outside [0, K)");
}

// Label expansion (ctc-loss.cc:116-129) with the sequence and expanded-label lengths, uploaded in stream order; the device
// pointers stay valid until the next call.
Ctc::Lattices Ctc::upload_lattices(const int* frame_num_utt, int S, const int* label_ids, const int* label_off) {
  int maxU = 0;
  for (int s = 0; s < S; ++s) {
    const int U = label_off[s + 1] - label_off[s];
    // an empty label sequence reads alpha column -1 in the reference (ctc-loss.cc:151); refuse it
    EESEN_REQUIRE(U >= 1, EESEN_ERR_INVALID, "every sequence needs at least one label");
    maxU = std::max(maxU, U);
  }
  const int Lprime = 2 * maxU + 1;  // ctc-loss.cc:118
  const int Lpad = lattice_pad(maxU);
  EESEN_REQUIRE(Lpad > 0, EESEN_ERR_INVALID, "expanded label length above 4096 (2047 labels per utterance) is not supported");

  // label expansion, sequence and expanded-label lengths: one stream-ordered upload (StageSlots)
  const size_t n_labx = (size_t)S * Lpad, n = n_labx + 2 * (size_t)S;
  if (labx.cap < n) EESEN_HIP_CHECK(hipStreamSynchronize(st));  // reallocation frees what queued kernels may still read
  labx.reserve(n);
  stage.upload(st, labx.p, n, [&](int* h) {
    for (int s = 0; s < S; ++s) {
      h[n_labx + s] = frame_num_utt[s];
      h[n_labx + S + s] = expand_labels(label_ids + label_off[s], label_off[s + 1] - label_off[s], h + (size_t)s * Lpad, Lpad);
    }
  });
  return Lattices{labx.p, labx.p + n_labx, labx.p + n_labx + S, Lpad, Lprime};
}

void Ctc::eval_parallel(const int* frame_num_utt, int S, const float* net_out, int rows, int K, int ld, const int* label_ids,
                        const int* label_off, float* diff, int ldd, float* pzx_host) {
  check_batch(frame_num_utt, S, rows, K, ld, label_ids, label_off);
  EESEN_REQUIRE(ldd >= K, EESEN_ERR_INVALID, "leading dimension smaller than the class count");
  EESEN_HIP_CHECK(hipSetDevice(device));
  const int T = rows / S;
  const Lattices lat = upload_lattices(frame_num_utt, S, label_ids, label_off);
  const int Lpad = lat.Lpad, Lprime = lat.Lprime;
  const int* labx_d = lat.labx;
  const int* lens_dd = lat.lens;
  const int* ll_d = lat.lablens;

  if (logp.cap < (size_t)rows * K || alpha.cap < (size_t)S * T * Lpad || pzx_d.cap < (size_t)S) EESEN_HIP_CHECK(hipStreamSynchronize(st));
  logp.reserve((size_t)rows * K);
  alpha.reserve((size_t)S * T * Lpad);
  beta.reserve((size_t)S * T * Lpad);
  pzx_d.reserve(S);

  clock.mark(st, 0);
  log_rows(st, net_out, ld, logp.p, K, rows, K);                                               // ctc-loss.cc:132-133
  clock.mark(st, 1);
  ctc_alpha_beta(st, logp.p, K, T, S, Lpad, labx_d, lens_dd, ll_d, alpha.p, beta.p, pzx_d.p, sweep_waves);  // :136-153
  clock.mark(st, 2);
  ctc_error_diff(st, net_out, ld, T, S, K, Lpad, Lprime, lens_dd, ll_d, labx_d, alpha.p, beta.p, pzx_d.p, diff, ldd);  // :156-168
  clock.stop(st);

  // ln p(z|x) per sequence (ctc-loss.cc:146-153 reads it element by element): back through a pinned slot.  A caller that wants
  // the values now waits for them; otherwise they join the objective sum when the next call needs the slot or the statistics.
  PendingPzx& q = ppzx[ppzx_idx++ & 1];
  flush_pzx(q);
  const float* pz = static_cast<const float*>(guard.read_back(q.pin, pzx_d.p, S * sizeof(float), st));
  q.S = S; q.active = true;
  q.nframes = 0;
  for (int s = 0; s < S; ++s) q.nframes += frame_num_utt[s];
  frames += q.nframes;
  sequences += S;
  if (pzx_host) {
    flush();  // keeps the accumulation order of the calls
    // a minibatch computed from a timed-out forward pass (guard word set) has no ln p: NaN, never garbage with status OK
    const bool bad = StatGuard::raised(pz, S * sizeof(float));
    for (int s = 0; s < S; ++s) pzx_host[s] = bad ? std::numeric_limits<float>::quiet_NaN() : pz[s];
  }
  last_lens.assign(frame_num_utt, frame_num_utt + S);
  last_T = T; last_S = S; last_Lpad = Lpad; last_Lprime = Lprime;
}

// Best-path alignment of every utterance against its labels.  The delta rows borrow `alpha`, the logarithms `logp`; the statistics
// and the accessors of the last EvalParallel (last_*) are left alone.
void Ctc::align_parallel(const int* frame_num_utt, int S, const float* scores, int rows, int K, int ld, bool is_log, const int* label_ids,
                         const int* label_off, int* ali_host, int* pos_host, float* score_host) {
  check_batch(frame_num_utt, S, rows, K, ld, label_ids, label_off);
  EESEN_HIP_CHECK(hipSetDevice(device));
  const int T = rows / S;
  const Lattices lat = upload_lattices(frame_num_utt, S, label_ids, label_off);
  const size_t n_out = 2 * (size_t)rows + S;   // class ids, positions, scores
  if ((!is_log && logp.cap < (size_t)rows * K) || alpha.cap < (size_t)S * T * lat.Lpad || ali_d.cap < n_out) EESEN_HIP_CHECK(hipStreamSynchronize(st));
  if (!is_log) logp.reserve((size_t)rows * K);
  alpha.reserve((size_t)S * T * lat.Lpad);
  ali_d.reserve(n_out);
  int* ali_dev = ali_d.p;
  int* pos_dev = ali_dev + rows;
  float* score_dev = reinterpret_cast<float*>(pos_dev + rows);

  align_clock.mark(st, 0);
  if (!is_log) log_rows(st, scores, ld, logp.p, K, rows, K);
  align_clock.mark(st, 1);
  ctc_best_path(st, is_log ? scores : logp.p, is_log ? ld : K, T, S, lat.Lpad, lat.labx, lat.lens, lat.lablens, alpha.p, sweep_waves);
  align_clock.mark(st, 2);
  ctc_traceback(st, alpha.p, T, S, lat.Lpad, lat.labx, lat.lens, lat.lablens, ali_dev, pos_dev, score_dev);
  align_clock.stop(st);

  const int* out = static_cast<const int*>(guard.read_back(align_pin, ali_dev, n_out * sizeof(int), st));
  align_pin.wait();
  const bool bad = StatGuard::raised(out, n_out * sizeof(int));   // no alignment: NaN and -1
  for (int r = 0; r < rows; ++r) {
    ali_host[r] = bad ? -1 : out[r];
    if (pos_host) pos_host[r] = bad ? -1 : out[rows + r];
  }
  const float* sc = reinterpret_cast<const float*>(out + 2 * (size_t)rows);
  for (int s = 0; s < S; ++s) score_host[s] = bad ? std::numeric_limits<float>::quiet_NaN() : sc[s];
}

// Prefix beam search of every utterance (INTEGRATION.md "Decoding").  The logarithms borrow `logp`; everything else is this call's own.
void Ctc::decode_parallel(const int* frame_num_utt, int S, const float* scores, int rows, int K, int ld, bool is_log, int beam, int max_classes,
                          int nbest, int* hyp_host, int* hyp_len_host, float* score_host) {
  decode_batch(frame_num_utt, S, scores, rows, K, ld, is_log, beam, max_classes, nbest, nullptr, nullptr, 0.f, 0.f, false, hyp_host, hyp_len_host, score_host,
               nullptr, nullptr, nullptr, nullptr);
}

// With a token LM fused into the beam (INTEGRATION.md "LM fusion"): ctc_prefix_beam with the tables, inside the same phase.  The
// tables are uploaded when this Ctc meets the model for the first time.
void Ctc::decode_parallel_lm(const int* frame_num_utt, int S, const float* scores, int rows, int K, int ld, bool is_log, int beam, int max_classes,
                             int nbest, const TokenLm* lm, float lm_weight, float insertion_bonus, bool use_eos, int* hyp_host, int* hyp_len_host,
                             float* score_host, float* lm_score_host) {
  EESEN_REQUIRE(lm != nullptr, EESEN_ERR_INVALID, "decoding with an LM: the LM handle is null");
  EESEN_REQUIRE(lm->K == K, EESEN_ERR_INVALID, "the LM was built for another class count K than the scores have");
  EESEN_REQUIRE(!use_eos || lm->has_eos, EESEN_ERR_INVALID, "use_eos on an LM whose file has no </s>");
  EESEN_REQUIRE(std::isfinite(lm_weight) && std::isfinite(insertion_bonus), EESEN_ERR_INVALID, "lm_weight and insertion_bonus must be finite");
  decode_batch(frame_num_utt, S, scores, rows, K, ld, is_log, beam, max_classes, nbest, nullptr, lm, lm_weight, insertion_bonus, use_eos, hyp_host,
               hyp_len_host, score_host, lm_score_host, nullptr, nullptr, nullptr);
}

// what the two lexicon searches ask of their lexicon and its word LM
static void check_lexicon(const Lexicon* lex, bool unspaced, const TokenLm* lm, int K, bool use_eos, float lm_weight, float word_bonus) {
  EESEN_REQUIRE(lex != nullptr, EESEN_ERR_INVALID, "decoding with a lexicon: the lexicon handle is null");
  if (unspaced) EESEN_REQUIRE(lex->unspaced, EESEN_ERR_INVALID, "a lexicon with a space class (eesen_lex_create) is decoded with eesen_ctc_decode_parallel_lex");
  else EESEN_REQUIRE(!lex->unspaced, EESEN_ERR_INVALID, "an unspaced lexicon (eesen_lex_create_unspaced) is decoded with eesen_ctc_decode_parallel_words");
  EESEN_REQUIRE(lex->K == K, EESEN_ERR_INVALID, "the lexicon was built for another class count K than the scores have");
  EESEN_REQUIRE(lm == nullptr || lm->K == lex->V() + 1, EESEN_ERR_INVALID, "the word LM's K must be the lexicon's word count + 1 (build it over eesen_lex_write_words' table)");
  EESEN_REQUIRE(!use_eos || (lm != nullptr && lm->has_eos), EESEN_ERR_INVALID, "use_eos without a word LM, or on one whose file has no </s>");
  EESEN_REQUIRE(std::isfinite(lm_weight) && std::isfinite(word_bonus), EESEN_ERR_INVALID, "lm_weight and word_bonus must be finite");
}

// Along a lexicon trie, with or without an LM over its words (INTEGRATION.md "Lexicon"): the same three launches; the lexicon's
// tables and the word LM's are uploaded when this Ctc meets them for the first time.  The words of every returned labelling are
// its segmentation, done here on the host.
void Ctc::decode_parallel_lex(const int* frame_num_utt, int S, const float* scores, int rows, int K, int ld, bool is_log, int beam, int max_classes,
                              int nbest, const Lexicon* lex, const TokenLm* lm, float lm_weight, float word_bonus, bool use_eos, int* hyp_host,
                              int* hyp_len_host, float* score_host, float* lm_score_host, int* word_host, int* word_len_host) {
  check_lexicon(lex, false, lm, K, use_eos, lm_weight, word_bonus);
  decode_batch(frame_num_utt, S, scores, rows, K, ld, is_log, beam, max_classes, nbest, lex, lm, lm_weight, word_bonus, use_eos, hyp_host, hyp_len_host,
               score_host, lm_score_host, nullptr, nullptr, nullptr);
  // (kept for decode_stamps, which speaks of these words and may run after the lexicon is gone: segmented whether asked for or not)
  const int T = rows / S;
  std::vector<int> w((size_t)T / 2 + 1);
  dec_word.assign((size_t)S * nbest * T, -1);
  dec_word_len.assign((size_t)S * nbest, -1);
  for (size_t i = 0; i < (size_t)S * nbest; ++i) {
    int nw = -1;   // (no entry, or a raised guard word)
    if (hyp_len_host[i] >= 0) {
      const bool in_language = lex->words(hyp_host + i * T, hyp_len_host[i], w.data(), &nw);
      EESEN_REQUIRE(in_language, EESEN_ERR_STATE, "decoding with a lexicon returned a labelling outside its language");
      std::copy(w.begin(), w.begin() + nw, dec_word.begin() + i * T);
    }
    dec_word_len[i] = nw;
    if (word_len_host) word_len_host[i] = nw;
    if (word_host)
      for (int j = 0; j < T; ++j) word_host[i * T + j] = j < nw ? w[j] : -1;
  }
}

void Ctc::upload_lex(const Lexicon& lex) {
  if (lex_serial == lex.serial) return;
  EESEN_HIP_CHECK(hipStreamSynchronize(st));   // (a launch in flight may still read the tables this replaces)
  const size_t nn = lex.word.size(), ne = lex.child_cls.size(), nw = lex.node_words.size();   // (nw: the unspaced kind's alone)
  std::vector<int> packed(4 * nn + 2 * ne + nw);
  for (size_t v = 0; v < nn; ++v) {
    int* r = packed.data() + 4 * v;
    r[0] = lex.first[v]; r[1] = lex.count[v];
    r[2] = lex.unspaced ? lex.wfirst[v] : lex.word[v];
    r[3] = lex.unspaced ? lex.wcount[v] : 0;
  }
  std::copy(lex.child_cls.begin(), lex.child_cls.end(), packed.begin() + 4 * nn);
  std::copy(lex.child_node.begin(), lex.child_node.end(), packed.begin() + 4 * nn + ne);
  std::copy(lex.node_words.begin(), lex.node_words.end(), packed.begin() + 4 * nn + 2 * ne);
  lex_i.reserve(packed.size());
  EESEN_HIP_CHECK(hipMemcpy(lex_i.p, packed.data(), packed.size() * sizeof(int), hipMemcpyHostToDevice));
  lex_tab = LexTables{lex_i.p, lex_i.p + 4 * nn, lex_i.p + 4 * nn + ne, lex.space};
  word_tab = WordLexTables{lex_i.p, lex_i.p + 4 * nn, lex_i.p + 4 * nn + ne, lex_i.p + 4 * nn + 2 * ne, lex.max_homophones, lex.K};
  lex_serial = lex.serial;
}

// The look-ahead table of (lex, lm) on the device, or null with the mode off.  Called behind upload_lex / upload_lm.
const float* Ctc::upload_lookahead(const Lexicon* lex, const TokenLm* lm) {
  if (lm_lookahead == 0) return nullptr;
  EESEN_REQUIRE(lm != nullptr, EESEN_ERR_INVALID, "the LM look-ahead (eesen_ctc_set_lm_lookahead) needs the word LM: decoding with a lexicon alone has nothing to look ahead to");
  if (la_lex_serial == lex->serial && la_lm_serial == lm->serial) return la_f.p;
  EESEN_HIP_CHECK(hipStreamSynchronize(st));   // (a launch in flight may still read the table this replaces)
  const size_t nn = (size_t)lex->nodes(), ne = lex->child_node.size();
  std::vector<float> la(nn + ne);   // behind the table: la of every edge's target, which the spaced search reads beside the target
  lex->lookahead(*lm, la.data());
  for (size_t e = 0; e < ne; ++e) la[nn + e] = la[lex->child_node[e]];
  la_f.reserve(la.size());
  EESEN_HIP_CHECK(hipMemcpy(la_f.p, la.data(), la.size() * sizeof(float), hipMemcpyHostToDevice));
  la_lex_serial = lex->serial;
  la_lm_serial = lm->serial;
  return la_f.p;
}

void Ctc::upload_lm(const TokenLm& lm) {
  if (lm_serial == lm.serial) return;
  EESEN_HIP_CHECK(hipStreamSynchronize(st));   // (a launch in flight may still read the tables this replaces)
  const size_t ns = lm.bo_w.size(), na = lm.arc_cls.size();
  std::vector<int> packed(4 * ns + 3 * na);
  auto bits = [](float v) { int b; std::memcpy(&b, &v, sizeof b); return b; };
  for (size_t i = 0; i < ns; ++i) {
    int* r = packed.data() + 4 * i;
    r[0] = lm.arc_off[i]; r[1] = lm.arc_off[i + 1] - lm.arc_off[i]; r[2] = lm.bo_next[i]; r[3] = bits(lm.bo_w[i]);
  }
  for (size_t i = 0; i < na; ++i) {
    packed[4 * ns + 2 * i] = bits(lm.arc_w[i]);
    packed[4 * ns + 2 * i + 1] = lm.arc_next[i];
    packed[4 * ns + 2 * na + i] = lm.arc_cls[i];
  }
  lm_i.reserve(packed.size());
  lm_f.reserve(ns);
  EESEN_HIP_CHECK(hipMemcpy(lm_i.p, packed.data(), packed.size() * sizeof(int), hipMemcpyHostToDevice));
  EESEN_HIP_CHECK(hipMemcpy(lm_f.p, lm.fin.data(), ns * sizeof(float), hipMemcpyHostToDevice));
  lm_tab = LmTables{lm_i.p, lm_i.p + 4 * ns, lm_i.p + 4 * ns + 2 * na, lm_f.p, lm.start};
  lm_serial = lm.serial;
}

// Every decode call: the checks, the buffers (DecodeLayout), the lengths, the logarithm and the top-C phase in front, the read-back
// behind.  In between the plain / fused search and its hypothesis kernel or, along an unspaced lexicon, the word search's, whose trie
// holds a third array and whose words, word ends and word counts come back behind the labels (the three hosts may be null).
void Ctc::decode_batch(const int* frame_num_utt, int S, const float* scores, int rows, int K, int ld, bool is_log, int beam, int max_classes,
                       int nbest, const Lexicon* lex, const TokenLm* lm, float lm_weight, float bonus, bool use_eos, int* hyp_host, int* hyp_len_host,
                       float* score_host, float* lm_score_host, int* word_host, int* word_len_host, int* word_end_host) {
  const bool words = lex && lex->unspaced;
  check_shape(frame_num_utt, S, rows, K, ld, words ? 0 : 2);   // (words: the lexicon's K is the scores', which its caller held)
  EESEN_REQUIRE(beam >= 1 && beam <= 64, EESEN_ERR_INVALID, "beam outside [1, 64]");
  EESEN_REQUIRE(max_classes >= 1 && max_classes <= 64, EESEN_ERR_INVALID, "max_classes outside [1, 64]");
  if (!words) EESEN_REQUIRE(beam * max_classes <= 2048, EESEN_ERR_INVALID, "beam * max_classes above 2048 (the candidate keys of a frame live in LDS)");
  else {
    const int H = lex->max_homophones;
    EESEN_REQUIRE((long)beam * (1 + (long)max_classes * (1 + H)) <= 4096, EESEN_ERR_INVALID,
                  "beam * (1 + max_classes * (1 + H)) above 4096, H = " + std::to_string(H) + " the lexicon's largest homophone set (the successor keys of a frame live in LDS)");
  }
  EESEN_REQUIRE(nbest >= 1 && nbest <= beam, EESEN_ERR_INVALID, "nbest outside [1, beam]");
  EESEN_HIP_CHECK(hipSetDevice(device));
  const DecodeLayout L = decode_layout(rows, S, K, beam, max_classes, nbest, words ? kDecodeWords : lm || lex ? kDecodeFused : kDecodePlain);
  const bool fused = L.fused();   // the beam carries LM sums (all 0 under a lexicon without an LM)
  EESEN_REQUIRE(L.n_trie <= ((size_t)1 << 30), EESEN_ERR_INVALID, "decoding: more than 2^30 trie nodes (S * (1 + T * beam)): decode fewer utterances together");
  if ((!is_log && logp.cap < (size_t)rows * K) || dec_f.cap < L.n_f || dec_i.cap < L.n_i || dec_trie.cap < L.n_t || dec_out.cap < L.n_out)
    EESEN_HIP_CHECK(hipStreamSynchronize(st));
  if (!is_log) logp.reserve((size_t)rows * K);
  dec_f.reserve(L.n_f);
  dec_i.reserve(L.n_i);
  dec_trie.reserve(L.n_t);
  dec_out.reserve(L.n_out);
  float *csc = dec_f.p + L.csc, *sblank = dec_f.p + L.sblank, *fscore = dec_f.p + L.fscore, *flm = fused ? dec_f.p + L.flm : nullptr;
  int *cid = dec_i.p + L.cid, *lens_d = dec_i.p + L.lens, *fnode = dec_i.p + L.fnode, *flen = dec_i.p + L.flen, *count = dec_i.p + L.count;
  int *trie0 = dec_trie.p + L.trie[0], *trie1 = dec_trie.p + L.trie[1], *out_d = dec_out.p;
  float* score_d = reinterpret_cast<float*>(out_d + L.score);
  float* lmsum_d = fused ? reinterpret_cast<float*>(out_d + L.lmsum) : nullptr;
  if (lm) upload_lm(*lm);
  if (lex) upload_lex(*lex);
  const float* la = lex ? upload_lookahead(lex, lm) : nullptr;   // (the plain and the token-LM search ignore the mode)
  stage.upload(st, lens_d, S, [&](int* pinned) { std::copy(frame_num_utt, frame_num_utt + S, pinned); });

  const float* sc = is_log ? scores : logp.p;
  const int sld = is_log ? ld : K, T = L.T, B = L.B, N = L.N;
  decode_clock.mark(st, 0);
  if (!is_log) log_rows(st, scores, ld, logp.p, K, rows, K);
  ctc_row_topc(st, sc, sld, rows, K, S, lens_d, L.C, cid, csc, sblank);
  decode_clock.mark(st, 1);
  if (words)
    ctc_word_beam(st, sc, sld, T, S, lens_d, B, L.C, cid, csc, sblank, lm ? &lm_tab : nullptr, word_tab, la, lm_weight, bonus, use_eos, trie0, trie1,
                  dec_trie.p + L.trie[2], fnode, flen, fscore, flm, dec_i.p + L.fword, dec_i.p + L.fnw, count);
  else
    ctc_prefix_beam(st, sc, sld, T, S, lens_d, B, L.C, cid, csc, sblank, lm ? &lm_tab : nullptr, lex ? &lex_tab : nullptr, la, la ? la + lex->nodes() : nullptr,
                    lm_weight, bonus, use_eos, trie0, trie1, fnode, flen, fscore, flm, count);
  decode_clock.mark(st, 2);
  if (words)
    ctc_word_hyp(st, trie0, trie1, dec_trie.p + L.trie[2], fnode, flen, fscore, flm, dec_i.p + L.fword, dec_i.p + L.fnw, count, T, S, B, N, out_d + L.hyp,
                 out_d + L.len, score_d, lmsum_d, out_d + L.words, out_d + L.ends, out_d + L.wlen);
  else
    ctc_hyp(st, trie0, trie1, fnode, flen, fscore, flm, count, T, S, B, N, out_d + L.hyp, out_d + L.len, score_d, lmsum_d);
  decode_clock.stop(st);
  dec = L;   // (decode_stamps, decode_rescore, decode_mbr: the hypotheses stay in dec_out and decode_pin)
  dec_lens.assign(frame_num_utt, frame_num_utt + S);
  dec_space = lex && !words ? lex->space : -1;
  dec_V = lex ? lex->V() : 0;

  const int* out = static_cast<const int*>(guard.read_back(decode_pin, out_d, L.n_out * sizeof(int), st));
  decode_pin.wait();
  const bool bad = StatGuard::raised(out, L.n_out * sizeof(int));   // no hypotheses: NaN and -1
  const float* outf = reinterpret_cast<const float*>(out);
  const float kNaN = std::numeric_limits<float>::quiet_NaN();
  for (size_t i = 0; i < L.n_hyp; ++i) {
    hyp_host[i] = bad ? -1 : out[L.hyp + i];
    if (word_host) word_host[i] = bad ? -1 : out[L.words + i];
    if (word_end_host) word_end_host[i] = bad ? -1 : out[L.ends + i];
  }
  for (size_t i = 0; i < L.NL; ++i) {
    hyp_len_host[i] = bad ? -1 : out[L.len + i];
    score_host[i] = bad ? kNaN : outf[L.score + i];
    if (fused && lm_score_host) lm_score_host[i] = bad ? kNaN : outf[L.lmsum + i];
    if (word_len_host) word_len_host[i] = bad ? -1 : out[L.wlen + i];
  }
}

// Along an unspaced lexicon (INTEGRATION.md "Words without a boundary unit"): decode_batch with the word beam and its hypothesis kernel.
// The final beam holds a word and a word count per hypothesis; nothing is segmented on the host.
void Ctc::decode_parallel_words(const int* frame_num_utt, int S, const float* scores, int rows, int K, int ld, bool is_log, int beam,
                                int max_classes, int nbest, const Lexicon* lex, const TokenLm* lm, float lm_weight, float word_bonus, bool use_eos,
                                int* hyp_host, int* hyp_len_host, float* score_host, float* lm_score_host, int* word_host, int* word_len_host,
                                int* word_end_host) {
  check_lexicon(lex, true, lm, K, use_eos, lm_weight, word_bonus);
  decode_batch(frame_num_utt, S, scores, rows, K, ld, is_log, beam, max_classes, nbest, lex, lm, lm_weight, word_bonus, use_eos, hyp_host, hyp_len_host,
               score_host, lm_score_host, word_host, word_len_host, word_end_host);
}

// N-best posterior word confidences (INTEGRATION.md "Time stamps and CTM"): lattice-to-ctm-conf's idea on a list instead of a lattice.
void word_confidence(int n, const double* scores, const int* word_len, const int* word_ids, const int* wstart, const int* wend, int stride,
                     double conf_scale, double* conf_out) {
  EESEN_REQUIRE(n >= 0 && stride >= 0, EESEN_ERR_INVALID, "word_confidence: negative entry count or stride");
  EESEN_REQUIRE(std::isfinite(conf_scale) && conf_scale >= 0, EESEN_ERR_INVALID, "conf_scale must be finite and >= 0");
  for (int i = 0; i < n; ++i)
    EESEN_REQUIRE(word_len[i] <= stride, EESEN_ERR_INVALID, "word_confidence: more words than the row holds");
  // P_i = exp(c (z_i - z_max)) / sum_k exp(c (z_k - z_max)): every exponent is <= 0 (the best entry's is 0), so nothing overflows
  double zmax = -std::numeric_limits<double>::infinity();
  for (int i = 0; i < n; ++i)
    if (word_len[i] >= 0) zmax = std::max(zmax, scores[i]);
  std::vector<double> P(n, 0.0);
  double sum = 0;
  for (int i = 0; i < n; ++i)
    if (word_len[i] >= 0) { P[i] = std::exp(conf_scale * (scores[i] - zmax)); sum += P[i]; }
  for (int i = 0; i < n; ++i) P[i] = sum > 0 ? P[i] / sum : 0.0;
  // every entry's words ordered by id: a word meets only the few of another entry that share its id (N-best lists of long
  // labellings: the all-pairs scan took longer than the alignment of the whole minibatch on the device)
  struct Occ { int id, b, e; };
  std::vector<std::vector<Occ>> by_id(n);
  for (int k = 0; k < n; ++k) {
    for (int m = 0; m < word_len[k]; ++m) {
      const size_t o = (size_t)k * stride + m;
      by_id[k].push_back(Occ{word_ids[o], wstart[o], wend[o]});
    }
    std::stable_sort(by_id[k].begin(), by_id[k].end(), [](const Occ& x, const Occ& y) { return x.id < y.id; });
  }
  for (int i = 0; i < n; ++i) {
    double* co = conf_out + (size_t)i * stride;
    for (int j = 0; j < stride; ++j) co[j] = -1e30;
    for (int j = 0; j < word_len[i]; ++j) {
      const int w = word_ids[(size_t)i * stride + j], b = wstart[(size_t)i * stride + j], e = wend[(size_t)i * stride + j];
      double c = 0;
      for (int k = 0; k < n; ++k) {   // in entry order: the sum's order is part of the result; each entry counts at most once
        auto it = std::lower_bound(by_id[k].begin(), by_id[k].end(), w, [](const Occ& x, int id) { return x.id < id; });
        bool hit = false;
        for (; it != by_id[k].end() && it->id == w && !hit; ++it) hit = it->b < e && b < it->e;
        if (hit) c += P[k];
      }
      co[j] = c;
    }
  }
}

// Time stamps of the last decode call's entries.  The hypotheses are where that call left them: labels and lengths in dec_out (device)
// and, with scores and words, in decode_pin (host); the frame counts behind the candidates in dec_i.  The delta rows borrow `alpha` as
// align_parallel's do, the logarithms `logp`.
void Ctc::decode_stamps(const int* frame_num_utt, int S, const float* scores, int rows, int K, int ld, bool is_log, double conf_scale,
                        int* lstart_host, int* lend_host, int* wstart_host, int* wend_host, float* wconf_host, float* path_score_host) {
  EESEN_REQUIRE(dec.rows > 0, EESEN_ERR_STATE, "time stamps: no decode call on this Ctc yet");
  EESEN_REQUIRE(S == dec.S && rows == dec.rows, EESEN_ERR_STATE, "time stamps: S or rows differ from the last decode call's");
  EESEN_REQUIRE(K > 0 && ld >= K, EESEN_ERR_INVALID, "leading dimension smaller than the class count");
  EESEN_REQUIRE(std::isfinite(conf_scale) && conf_scale >= 0, EESEN_ERR_INVALID, "conf_scale must be finite and >= 0");
  for (int s = 0; s < S; ++s)
    EESEN_REQUIRE(frame_num_utt[s] == dec_lens[s], EESEN_ERR_STATE, "time stamps: frame_num_utt differs from the last decode call's");
  EESEN_HIP_CHECK(hipSetDevice(device));
  const int T = dec.T, N = dec.N, tokens = dec_tokens();
  const size_t NL = dec.NL, n_hyp = dec.n_hyp;
  const int* dout = decode_pin.as<int>();
  const int* hyp_h = dout + dec.hyp;
  const int* hlen = dout + dec.len;
  const float* z = reinterpret_cast<const float*>(dout) + dec.score;
  const float kNaN = std::numeric_limits<float>::quiet_NaN();
  auto fill = [&](int* p, size_t n, int v) { if (p) std::fill(p, p + n, v); };
  auto fillf = [&](float* p, size_t n, float v) { if (p) std::fill(p, p + n, v); };
  auto all_bad = [&] {   // decoded or aligned from a timed-out forward pass (guard word set): -1 and NaN, never garbage with status OK
    fill(lstart_host, n_hyp, -1); fill(lend_host, n_hyp, -1); fill(wstart_host, n_hyp, -1); fill(wend_host, n_hyp, -1);
    fillf(wconf_host, n_hyp, kNaN); fillf(path_score_host, NL, kNaN);
  };
  if (StatGuard::raised(dout, dec.n_out * sizeof(int))) { all_bad(); return; }

  constexpr int kMaxLabels = kMaxLatticeLabels;   // an entry beyond has no lattice (ctc_hyp_lattices) and no stamps
  int maxU = 0;
  for (size_t i = 0; i < NL; ++i)
    if (hlen[i] <= kMaxLabels) maxU = std::max(maxU, hlen[i]);
  const int Lpad = lattice_pad(maxU);
  const size_t per_lattice = (size_t)T * Lpad;
  size_t G = stamp_group > 0 ? (size_t)stamp_group : std::max<size_t>(1, kStampDeltaBytes / (per_lattice * sizeof(float)));
  G = std::min(G, NL);

  const size_t n_res = 2 * n_hyp + NL;   // label starts, label ends, path scores
  const size_t n_int = NL * Lpad + 2 * NL + 2 * n_hyp + n_res;
  if ((!is_log && logp.cap < (size_t)rows * K) || alpha.cap < G * per_lattice || stamp_i.cap < n_int) EESEN_HIP_CHECK(hipStreamSynchronize(st));
  if (!is_log) logp.reserve((size_t)rows * K);
  alpha.reserve(G * per_lattice);
  stamp_i.reserve(n_int);
  int* labx_d = stamp_i.p;
  int* ll_d = labx_d + NL * Lpad;
  int* lens_l = ll_d + NL;
  int* pos_d = lens_l + NL;
  int* ali_d2 = pos_d + n_hyp;
  int* lstart_d = ali_d2 + n_hyp;
  int* lend_d = lstart_d + n_hyp;
  float* score_d = reinterpret_cast<float*>(lend_d + n_hyp);

  stamp_clock.mark(st, 0);
  if (!is_log) log_rows(st, scores, ld, logp.p, K, rows, K);
  ctc_hyp_lattices(st, dec_out.p + dec.hyp, dec_out.p + dec.len, dec_i.p + dec.lens, T, (int)NL, N, Lpad, labx_d, ll_d, lens_l);
  stamp_clock.mark(st, 1);
  for (size_t g0 = 0; g0 < NL; g0 += G) {   // groups of lattices: the delta rows stay within their budget
    const int gc = (int)std::min(G, NL - g0);
    ctc_best_path(st, is_log ? scores : logp.p, is_log ? ld : K, T, S, Lpad, labx_d + g0 * Lpad, lens_l + g0, ll_d + g0, alpha.p, sweep_waves, gc,
                  (int)g0, N);
    ctc_traceback(st, alpha.p, T, gc, Lpad, labx_d + g0 * Lpad, lens_l + g0, ll_d + g0, ali_d2 + g0 * T, pos_d + g0 * T, score_d + g0);
  }
  stamp_clock.mark(st, 2);
  ctc_stamp(st, pos_d, T, (int)NL, (int)G, lens_l, lstart_d, lend_d);
  stamp_clock.stop(st);

  const int* out = static_cast<const int*>(guard.read_back(stamp_pin, lstart_d, n_res * sizeof(int), st));
  stamp_pin.wait();
  if (StatGuard::raised(out, n_res * sizeof(int))) { all_bad(); return; }
  const int* ls = out;
  const int* le = out + n_hyp;
  const float* ps = reinterpret_cast<const float*>(out + 2 * n_hyp);

  // words: runs of labels [a, b] with an id, per entry; then the confidences per utterance
  std::vector<int> wid((size_t)N * T), wb((size_t)N * T), we((size_t)N * T), wl(N);
  std::vector<double> zz(N), conf((size_t)N * T);
  const bool want_words = wstart_host || wend_host || wconf_host;   // (a caller after the label intervals alone pays for neither)
  for (int s = 0; s < S; ++s) {
    for (int r = 0; r < N; ++r) {
      const size_t i = (size_t)s * N + r;
      const int U = hlen[i];
      const bool stamped = U >= 1 && U <= kMaxLabels;
      if (path_score_host) path_score_host[i] = U == 0 ? 0.f : stamped ? ps[i] : -1e30f;
      for (int t = 0; t < T; ++t) {
        if (lstart_host) lstart_host[i * T + t] = stamped ? ls[i * T + t] : -1;
        if (lend_host) lend_host[i * T + t] = stamped ? le[i * T + t] : -1;
      }
      if (!want_words) continue;
      int* id = wid.data() + (size_t)r * T;
      int* b = wb.data() + (size_t)r * T;
      int* e = we.data() + (size_t)r * T;
      std::fill(id, id + T, -1); std::fill(b, b + T, -1); std::fill(e, e + T, -1);
      int nw = U < 0 ? -1 : 0;
      auto word = [&](int w, int first, int last) {   // labels [first, last] are word w
        id[nw] = w;
        b[nw] = stamped ? ls[i * T + first] : -1;
        e[nw] = stamped ? le[i * T + last] : -1;
        ++nw;
      };
      const int* h = hyp_h + i * T;
      if (tokens == 0) {
        for (int u = 0; u < U; ++u) word(h[u], u, u);
      } else if (tokens == 1) {
        const int want = dec_word_len[i];   // the runs between the space labels, whose frames belong to no word
        int first = 0;
        for (int u = 0; u <= U && U > 0; ++u) {
          if (u < U && h[u] != dec_space) continue;
          EESEN_REQUIRE(u > first && nw < want, EESEN_ERR_STATE, "time stamps: the labelling's spaces do not match its words");
          word(dec_word[i * T + nw], first, u - 1);
          first = u + 1;
        }
        EESEN_REQUIRE(nw == want, EESEN_ERR_STATE, "time stamps: the labelling's spaces do not match its words");
      } else {
        const int want = dout[dec.wlen + i];
        int first = 0;
        for (int j = 0; j < want && j < T; ++j) {
          const int end = dout[dec.ends + i * T + j];
          EESEN_REQUIRE(end > first && end <= U, EESEN_ERR_STATE, "time stamps: word ends outside the labelling");
          word(dout[dec.words + i * T + j], first, end - 1);
          first = end;
        }
      }
      wl[r] = nw;
      zz[r] = z[i];
    }
    if (!want_words) continue;
    if (wconf_host) word_confidence(N, zz.data(), wl.data(), wid.data(), wb.data(), we.data(), T, conf_scale, conf.data());
    for (int r = 0; r < N; ++r) {
      const size_t i = (size_t)s * N + r;
      for (int t = 0; t < T; ++t) {
        if (wstart_host) wstart_host[i * T + t] = wb[(size_t)r * T + t];
        if (wend_host) wend_host[i * T + t] = we[(size_t)r * T + t];
        if (wconf_host) wconf_host[i * T + t] = (float)conf[(size_t)r * T + t];
      }
    }
  }
}

// Exact log-scores of labellings given by the host (INTEGRATION.md "Rescoring").  The lattices are expanded here and uploaded as
// upload_lattices does, into buffers of this call's own: labx, alpha and the last_* accessors of eval_parallel stay as they are.
void Ctc::score_parallel(const int* frame_num_utt, int S, const float* scores, int rows, int K, int ld, bool is_log, const int* hyp_off,
                         const int* label_off, const int* label_ids, float* score_host) {
  check_shape(frame_num_utt, S, rows, K, ld, 0);
  const int T = rows / S;
  EESEN_REQUIRE(hyp_off[0] == 0, EESEN_ERR_INVALID, "hyp_off must start at 0");
  for (int s = 0; s < S; ++s)
    EESEN_REQUIRE(hyp_off[s + 1] >= hyp_off[s], EESEN_ERR_INVALID, "labelling offsets must be non-decreasing");
  const int NH = hyp_off[S];
  int maxU = 0;
  for (int h = 0; h < NH; ++h) {
    EESEN_REQUIRE(label_off[h + 1] >= label_off[h], EESEN_ERR_INVALID, "label offsets must be non-decreasing");
    maxU = std::max(maxU, label_off[h + 1] - label_off[h]);
  }
  const int Lpad = lattice_pad(maxU);
  EESEN_REQUIRE(Lpad > 0, EESEN_ERR_INVALID, "expanded label length above 4096 (2047 labels per labelling) is not supported");
  if (NH > 0)
    for (int i = label_off[0]; i < label_off[NH]; ++i)
      EESEN_REQUIRE(label_ids[i] >= 1 && label_ids[i] < K, EESEN_ERR_INVALID, "label id outside [1, K)");
  if (NH == 0) return;
  EESEN_HIP_CHECK(hipSetDevice(device));

  const size_t n_labx = (size_t)NH * Lpad, n_in = n_labx + 3 * (size_t)NH, n_int = n_in + NH;
  if ((!is_log && logp.cap < (size_t)rows * K) || score_i.cap < n_int) EESEN_HIP_CHECK(hipStreamSynchronize(st));
  if (!is_log) logp.reserve((size_t)rows * K);
  score_i.reserve(n_int);
  int* labx_d = score_i.p;
  int* ll_d = labx_d + n_labx;
  int* lens_l = ll_d + NH;
  int* utt_d = lens_l + NH;
  float* score_d = reinterpret_cast<float*>(utt_d + NH);
  stage.upload(st, labx_d, n_in, [&](int* h) {   // every labelling's lattice, expanded length, frame count and utterance
    for (int s = 0; s < S; ++s)
      for (int q = hyp_off[s]; q < hyp_off[s + 1]; ++q) {
        h[n_labx + q] = expand_labels(label_ids + label_off[q], label_off[q + 1] - label_off[q], h + (size_t)q * Lpad, Lpad);
        h[n_labx + NH + q] = frame_num_utt[s];
        h[n_labx + 2 * (size_t)NH + q] = s;
      }
  });

  rescore_clock.mark(st, 0);
  if (!is_log) log_rows(st, scores, ld, logp.p, K, rows, K);
  rescore_clock.mark(st, 1);
  ctc_score(st, is_log ? scores : logp.p, is_log ? ld : K, T, S, NH, Lpad, labx_d, lens_l, ll_d, utt_d, score_d, sweep_waves);
  rescore_clock.stop(st);
  rescore_host_s = 0;

  const float* out = static_cast<const float*>(guard.read_back(score_pin, score_d, (size_t)NH * sizeof(float), st));
  score_pin.wait();
  const bool bad = StatGuard::raised(out, (size_t)NH * sizeof(float));   // no scores: NaN
  if (score_host)
    for (int h = 0; h < NH; ++h) score_host[h] = bad ? std::numeric_limits<float>::quiet_NaN() : out[h];
}

// Second pass over the last decode call's entries.  The hypotheses are where decode_stamps finds them; their lattices are built on
// the device (ctc_hyp_lattices in its scoring form) and swept in one launch; the LM scores and the ranking are the host's.
void Ctc::decode_rescore(const int* frame_num_utt, int S, const float* scores, int rows, int K, int ld, bool is_log, const TokenLm* lm,
                         float lm_weight, float bonus, bool use_eos, float* am_host, float* lm_host, float* total_host, int* order_host) {
  EESEN_REQUIRE(dec.rows > 0, EESEN_ERR_STATE, "rescoring: no decode call on this Ctc yet");
  EESEN_REQUIRE(S == dec.S && rows == dec.rows, EESEN_ERR_STATE, "rescoring: S or rows differ from the last decode call's");
  EESEN_REQUIRE(K > 0 && ld >= K, EESEN_ERR_INVALID, "leading dimension smaller than the class count");
  EESEN_REQUIRE(std::isfinite(lm_weight) && std::isfinite(bonus), EESEN_ERR_INVALID, "lm_weight and bonus must be finite");
  if (lm) {
    EESEN_REQUIRE(!use_eos || lm->has_eos, EESEN_ERR_INVALID, "use_eos on an LM whose file has no </s>");
    if (dec_tokens() == 0) EESEN_REQUIRE(lm->K == K, EESEN_ERR_INVALID, "the rescoring LM was built for another class count K than the scores have");
    else EESEN_REQUIRE(lm->K == dec_V + 1, EESEN_ERR_INVALID, "the rescoring word LM's K must be the lexicon's word count + 1");
  }
  for (int s = 0; s < S; ++s)
    EESEN_REQUIRE(frame_num_utt[s] == dec_lens[s], EESEN_ERR_STATE, "rescoring: frame_num_utt differs from the last decode call's");
  EESEN_HIP_CHECK(hipSetDevice(device));
  const int T = dec.T, N = dec.N, tokens = dec_tokens();
  const size_t NL = dec.NL;
  const int* dout = decode_pin.as<int>();
  const int* hlen = dout + dec.len;
  const float* lmsum = reinterpret_cast<const float*>(dout) + dec.lmsum;   // (fused: the first pass's LM sums)
  const float kNaN = std::numeric_limits<float>::quiet_NaN();
  auto all_bad = [&] {   // decoded or scored from a timed-out forward pass (guard word set): NaN and -1, never garbage with status OK
    if (am_host) std::fill(am_host, am_host + NL, kNaN);
    if (lm_host) std::fill(lm_host, lm_host + NL, kNaN);
    if (total_host) std::fill(total_host, total_host + NL, kNaN);
    if (order_host) std::fill(order_host, order_host + NL, -1);
  };
  if (StatGuard::raised(dout, dec.n_out * sizeof(int))) { all_bad(); return; }

  int maxU = 0;   // (an entry beyond kMaxLatticeLabels has no lattice (ctc_hyp_lattices) and reads as infeasible)
  for (size_t i = 0; i < NL; ++i)
    if (hlen[i] <= kMaxLatticeLabels) maxU = std::max(maxU, hlen[i]);
  const int Lpad = lattice_pad(maxU);
  const size_t n_int = NL * Lpad + 4 * NL;
  if ((!is_log && logp.cap < (size_t)rows * K) || score_i.cap < n_int) EESEN_HIP_CHECK(hipStreamSynchronize(st));
  if (!is_log) logp.reserve((size_t)rows * K);
  score_i.reserve(n_int);
  int* labx_d = score_i.p;
  int* ll_d = labx_d + NL * Lpad;
  int* lens_l = ll_d + NL;
  int* utt_d = lens_l + NL;
  float* score_d = reinterpret_cast<float*>(utt_d + NL);

  rescore_clock.mark(st, 0);
  if (!is_log) log_rows(st, scores, ld, logp.p, K, rows, K);
  ctc_hyp_lattices(st, dec_out.p + dec.hyp, dec_out.p + dec.len, dec_i.p + dec.lens, T, (int)NL, N, Lpad, labx_d, ll_d, lens_l, utt_d);
  rescore_clock.mark(st, 1);
  ctc_score(st, is_log ? scores : logp.p, is_log ? ld : K, T, S, (int)NL, Lpad, labx_d, lens_l, ll_d, utt_d, score_d, sweep_waves);
  rescore_clock.stop(st);

  const float* out = static_cast<const float*>(guard.read_back(score_pin, score_d, NL * sizeof(float), st));
  score_pin.wait();
  if (StatGuard::raised(out, NL * sizeof(float))) { all_bad(); return; }

  const auto t0 = std::chrono::steady_clock::now();
  std::vector<float> tot(N);
  std::vector<int> ord(N);
  for (int s = 0; s < S; ++s) {
    int nf = 0;   // feasible entries, in first-pass rank order
    for (int r = 0; r < N; ++r) {
      const size_t i = (size_t)s * N + r;
      const int U = hlen[i];
      const float a = out[i];
      const bool feasible = U >= 0 && a > -1e29f;
      float g32 = -1e30f;
      tot[r] = -1e30f;
      if (feasible) {
        const int* tok = tokens == 0 ? dout + dec.hyp + i * T : tokens == 1 ? dec_word.data() + i * T : dout + dec.words + i * T;
        const int n = tokens == 0 ? U : tokens == 1 ? dec_word_len[i] : dout[dec.wlen + i];
        const double g = lm ? lm->score(tok, n, use_eos, nullptr) : dec.fused() ? (double)lmsum[i] : 0.0;
        g32 = (float)g;
        tot[r] = (float)((double)a + (double)lm_weight * g + (double)bonus * n);
        ord[nf++] = r;
      }
      if (am_host) am_host[i] = feasible ? a : -1e30f;
      if (lm_host) lm_host[i] = g32;
      if (total_host) total_host[i] = tot[r];
    }
    // by total, descending; a tie keeps the first-pass order; then the entries without a score, in rank order
    std::stable_sort(ord.begin(), ord.begin() + nf, [&](int x, int y) { return tot[x] > tot[y]; });
    std::vector<char> placed(N, 0);
    for (int k = 0; k < nf; ++k) placed[ord[k]] = 1;
    for (int r = 0; r < N; ++r)
      if (!placed[r]) ord[nf++] = r;
    if (order_host) std::copy(ord.begin(), ord.end(), order_host + (size_t)s * N);
  }
  rescore_host_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

namespace {
double seconds_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
}  // namespace

const int* Ctc::ed_run(const int* tok_h, size_t n_tok, const int* dev_tok, const std::vector<int>& jobs, size_t n_same, int max_len, bool* bad) {
  const auto t0 = std::chrono::steady_clock::now();
  const size_t nj = jobs.size() / 4, n_in = n_tok + 4 * nj, n_all = n_in + nj;
  EESEN_REQUIRE(n_all < ((size_t)1 << 31), EESEN_ERR_INVALID, "edit distances: more than 2^31 tokens and jobs in one call");
  EESEN_HIP_CHECK(hipSetDevice(device));
  if (ed_i.cap < n_all) EESEN_HIP_CHECK(hipStreamSynchronize(st));
  ed_i.reserve(std::max<size_t>(n_all, 1));
  int* tok_d = ed_i.p;
  int* jobs_d = tok_d + n_tok;
  int* out_d = jobs_d + 4 * nj;
  if (n_in > 0)
    stage.upload(st, tok_d, n_in, [&](int* pinned) {
      if (n_tok > 0) std::copy(tok_h, tok_h + n_tok, pinned);
      std::copy(jobs.begin(), jobs.end(), pinned + n_tok);
    });
  const double build_s = seconds_since(t0);
  if (nj > 0) {
    const int* first = dev_tok ? dev_tok : tok_d;
    n_same = std::min(n_same, nj);
    mev[0].record(st);
    if (!dev_tok) edit_distance_jobs(st, tok_d, tok_d, jobs_d, (int)nj, max_len, out_d);
    else {
      edit_distance_jobs(st, first, first, jobs_d, (int)n_same, max_len, out_d);
      edit_distance_jobs(st, first, tok_d, jobs_d + 4 * n_same, (int)(nj - n_same), max_len, out_d + n_same);
    }
    mev[1].record(st);
  }
  // (bad == null: the tokens are the caller's, no forward pass to guard)
  const int* out = static_cast<const int*>(guard.read_back(ed_pin, out_d, nj * sizeof(int), st, bad != nullptr));
  ed_pin.wait();
  if (bad) *bad = StatGuard::raised(out, nj * sizeof(int));
  float ms = 0.f;
  if (nj > 0) EESEN_HIP_CHECK(hipEventElapsedTime(&ms, mev[0], mev[1]));
  mbr_t[0] += build_s;
  mbr_t[1] += ms * 1e-3;
  return out;
}

// Distances among and from sequences given by the host (INTEGRATION.md "Minimum Bayes risk").  Every group's pairs i < j are one job
// each and mirrored here; a sequence against its group's reference is one more.
void Ctc::edit_distance_parallel(int G, const int* seq_off, const int* tok_off, const int* tok_ids, const int* ref_off, const int* ref_ids,
                                 int* pair_host, int* ref_dist_host) {
  const auto t0 = std::chrono::steady_clock::now();
  EESEN_REQUIRE(seq_off[0] == 0, EESEN_ERR_INVALID, "seq_off must start at 0");
  for (int g = 0; g < G; ++g) EESEN_REQUIRE(seq_off[g + 1] >= seq_off[g], EESEN_ERR_INVALID, "sequence offsets must be non-decreasing");
  const int NQ = seq_off[G];
  int max_len = 0;
  for (int q = 0; q < NQ; ++q) {
    const int n = tok_off[q + 1] - tok_off[q];
    EESEN_REQUIRE(n >= 0, EESEN_ERR_INVALID, "token offsets must be non-decreasing");
    EESEN_REQUIRE(n <= kEditDistanceMaxLen, EESEN_ERR_INVALID, "a sequence of more than 8192 tokens is not supported");
    max_len = std::max(max_len, n);
  }
  const bool refs = ref_off != nullptr;
  if (refs)
    for (int g = 0; g < G; ++g) {
      const int n = ref_off[g + 1] - ref_off[g];
      EESEN_REQUIRE(n >= 0, EESEN_ERR_INVALID, "reference offsets must be non-decreasing");
      EESEN_REQUIRE(n <= kEditDistanceMaxLen, EESEN_ERR_INVALID, "a reference of more than 8192 tokens is not supported");
      max_len = std::max(max_len, n);
    }
  const size_t n_seq_tok = NQ > 0 ? (size_t)(tok_off[NQ] - tok_off[0]) : 0, n_ref_tok = refs ? (size_t)(ref_off[G] - ref_off[0]) : 0;
  EESEN_REQUIRE(n_seq_tok == 0 || tok_ids != nullptr, EESEN_ERR_INVALID, "tok_ids is null");
  EESEN_REQUIRE(n_ref_tok == 0 || ref_ids != nullptr, EESEN_ERR_INVALID, "ref_ids is null");
  if (!mbr_accumulate) mbr_t[0] = mbr_t[1] = mbr_t[2] = 0;
  if (NQ == 0) return;
  std::vector<int> tok(n_seq_tok + n_ref_tok);
  if (n_seq_tok) std::copy(tok_ids + tok_off[0], tok_ids + tok_off[NQ], tok.begin());
  if (n_ref_tok) std::copy(ref_ids + ref_off[0], ref_ids + ref_off[G], tok.begin() + n_seq_tok);
  std::vector<int> jobs;
  auto span = [&](int q, int* off, int* len) { *off = tok_off[q] - tok_off[0]; *len = tok_off[q + 1] - tok_off[q]; };
  size_t n_pairs = 0;
  if (pair_host)
    for (int g = 0; g < G; ++g)
      for (int i = seq_off[g]; i < seq_off[g + 1]; ++i)
        for (int j = i + 1; j < seq_off[g + 1]; ++j) {
          int oa, la, ob, lb;
          span(i, &oa, &la); span(j, &ob, &lb);
          jobs.insert(jobs.end(), {oa, la, ob, lb});
          ++n_pairs;
        }
  if (refs && ref_dist_host)
    for (int g = 0; g < G; ++g)
      for (int i = seq_off[g]; i < seq_off[g + 1]; ++i) {
        int oa, la;
        span(i, &oa, &la);
        jobs.insert(jobs.end(), {oa, la, (int)n_seq_tok + ref_off[g] - ref_off[0], ref_off[g + 1] - ref_off[g]});
      }
  mbr_t[0] += seconds_since(t0);
  const int* d = ed_run(tok.data(), tok.size(), nullptr, jobs, jobs.size() / 4, max_len, nullptr);   // (no guard: the tokens are the caller's)
  const auto t1 = std::chrono::steady_clock::now();
  if (pair_host) {
    size_t k = 0;
    int* out = pair_host;
    for (int g = 0; g < G; ++g) {
      const int n = seq_off[g + 1] - seq_off[g];
      for (int i = 0; i < n; ++i) {
        out[(size_t)i * n + i] = 0;
        for (int j = i + 1; j < n; ++j) out[(size_t)i * n + j] = out[(size_t)j * n + i] = d[k++];
      }
      out += (size_t)n * n;
    }
  }
  if (refs && ref_dist_host) std::copy(d + n_pairs, d + n_pairs + NQ, ref_dist_host);
  mbr_t[2] += seconds_since(t1);
}

// Minimum Bayes risk over the last decode call's entries.  The tokens are where that call left them: labels and the unspaced mode's
// words in dec_out (device), the spaced mode's words in dec_word (host, uploaded); lengths and scores in decode_pin.
void Ctc::decode_mbr(int S, int level, double scale, const float* total_host, const int* ref_off, const int* ref_ids, int* dist_host,
                     int* ref_dist_host, double* post_host, double* risk_host, int* order_host) {
  const auto t0 = std::chrono::steady_clock::now();
  EESEN_REQUIRE(dec.rows > 0, EESEN_ERR_STATE, "MBR: no decode call on this Ctc yet");
  EESEN_REQUIRE(S == dec.S, EESEN_ERR_STATE, "MBR: S differs from the last decode call's");
  EESEN_REQUIRE(level == 0 || level == 1, EESEN_ERR_INVALID, "MBR: level must be 0 (LM tokens) or 1 (labels)");
  EESEN_REQUIRE(std::isfinite(scale) && scale >= 0, EESEN_ERR_INVALID, "MBR: scale must be finite and >= 0");
  const bool refs = ref_off != nullptr;
  int max_len = 0;
  if (refs) {
    for (int s = 0; s < S; ++s) {
      const int n = ref_off[s + 1] - ref_off[s];
      EESEN_REQUIRE(n >= 0, EESEN_ERR_INVALID, "reference offsets must be non-decreasing");
      EESEN_REQUIRE(n <= kEditDistanceMaxLen, EESEN_ERR_INVALID, "a reference of more than 8192 tokens is not supported");
      max_len = std::max(max_len, n);
    }
    EESEN_REQUIRE(ref_off[S] == ref_off[0] || ref_ids != nullptr, EESEN_ERR_INVALID, "ref_ids is null");
  }
  if (!mbr_accumulate) mbr_t[0] = mbr_t[1] = mbr_t[2] = 0;
  const int T = dec.T, N = dec.N;
  const size_t NL = dec.NL;
  const int* dout = decode_pin.as<int>();
  const int* hlen = dout + dec.len;
  const float* z32 = total_host ? total_host : reinterpret_cast<const float*>(dout) + dec.score;
  const double kNaN = std::numeric_limits<double>::quiet_NaN();
  auto all_bad = [&] {   // decoded from a timed-out forward pass (guard word set): -1 and NaN, never garbage with status OK
    if (dist_host) std::fill(dist_host, dist_host + NL * N, -1);
    if (ref_dist_host) std::fill(ref_dist_host, ref_dist_host + NL, -1);
    if (post_host) std::fill(post_host, post_host + NL, kNaN);
    if (risk_host) std::fill(risk_host, risk_host + NL, kNaN);
    if (order_host) std::fill(order_host, order_host + NL, -1);
  };
  if (StatGuard::raised(dout, dec.n_out * sizeof(int))) { all_bad(); return; }

  // every entry's tokens: where they are and how many; the entries that count
  const int kind = level == 1 ? 0 : dec_tokens();   // 0 labels, 1 the spaced mode's words, 2 the unspaced mode's
  std::vector<int> off(NL), len(NL), tok;       // (tok: the uploaded tokens -- the spaced mode's words, then the references)
  std::vector<char> counts(NL);
  for (size_t i = 0; i < NL; ++i) {
    const int n = hlen[i] < 0 ? -1 : kind == 0 ? hlen[i] : kind == 1 ? dec_word_len[i] : dout[dec.wlen + i];
    const float z = z32[i];
    counts[i] = n >= 0 && n <= kEditDistanceMaxLen && z > -1e29f && !std::isnan(z);
    len[i] = n;
    if (kind == 1) {
      off[i] = (int)tok.size();
      if (counts[i]) tok.insert(tok.end(), dec_word.begin() + i * T, dec_word.begin() + i * T + n);
    } else {
      EESEN_REQUIRE(i * T + (kind == 2 ? dec.words : 0) < ((size_t)1 << 31), EESEN_ERR_INVALID, "MBR: hypothesis buffer beyond 2^31 ints");
      off[i] = (int)(i * T);
    }
    if (counts[i]) max_len = std::max(max_len, n);
  }
  const int* dev_tok = kind == 0 ? dec_out.p + dec.hyp : kind == 2 ? dec_out.p + dec.words : nullptr;
  const int ref_base = (int)tok.size();
  if (refs && ref_off[S] > ref_off[0]) tok.insert(tok.end(), ref_ids + ref_off[0], ref_ids + ref_off[S]);
  const bool need_pairs = dist_host || risk_host || order_host, need_ref = refs && ref_dist_host;
  std::vector<int> jobs;
  size_t n_pairs = 0;
  if (need_pairs)
    for (int s = 0; s < S; ++s)
      for (int i = 0; i < N; ++i)
        for (int k = i + 1; k < N; ++k) {
          const size_t a = (size_t)s * N + i, b = (size_t)s * N + k;
          if (!counts[a] || !counts[b]) continue;
          jobs.insert(jobs.end(), {off[a], len[a], off[b], len[b]});
          ++n_pairs;
        }
  if (need_ref)
    for (size_t i = 0; i < NL; ++i)
      if (counts[i]) jobs.insert(jobs.end(), {off[i], len[i], ref_base + ref_off[i / N] - ref_off[0], ref_off[i / N + 1] - ref_off[i / N]});
  mbr_t[0] += seconds_since(t0);
  bool bad = false;
  const int* d = ed_run(tok.data(), tok.size(), dev_tok, jobs, n_pairs, max_len, &bad);
  if (bad) { all_bad(); return; }

  const auto t1 = std::chrono::steady_clock::now();
  std::vector<int> D((size_t)N * N), ord(N);
  std::vector<double> P(N), R(N);
  size_t kp = 0, kr = n_pairs;
  for (int s = 0; s < S; ++s) {
    const char* cnt = counts.data() + (size_t)s * N;
    const float* z = z32 + (size_t)s * N;
    std::fill(D.begin(), D.end(), -1);
    if (need_pairs)
      for (int i = 0; i < N; ++i) {
        if (!cnt[i]) continue;
        D[(size_t)i * N + i] = 0;
        for (int k = i + 1; k < N; ++k)
          if (cnt[k]) D[(size_t)i * N + k] = D[(size_t)k * N + i] = d[kp++];
      }
    if (dist_host) std::copy(D.begin(), D.end(), dist_host + (size_t)s * N * N);
    if (ref_dist_host)
      for (int i = 0; i < N; ++i) ref_dist_host[(size_t)s * N + i] = need_ref && cnt[i] ? d[kr++] : -1;
    // P_i = exp(c (z_i - z_max)) / sum_k exp(c (z_k - z_max)) over the counting entries in rank order: every exponent is <= 0
    double zmax = -std::numeric_limits<double>::infinity(), sum = 0;
    for (int i = 0; i < N; ++i)
      if (cnt[i]) zmax = std::max(zmax, (double)z[i]);
    for (int i = 0; i < N; ++i) {
      P[i] = cnt[i] ? std::exp(scale * ((double)z[i] - zmax)) : 0.0;
      if (cnt[i]) sum += P[i];
    }
    int nc = 0;
    for (int i = 0; i < N; ++i)
      if (cnt[i]) { P[i] = P[i] / sum; ord[nc++] = i; }
    // risk_i = sum_k P_k d(i, k), over the counting k in rank order
    for (int i = 0; i < N; ++i) {
      double r = 0;
      if (cnt[i] && need_pairs)
        for (int k = 0; k < N; ++k)
          if (cnt[k]) r += P[k] * (double)D[(size_t)i * N + k];
      R[i] = r;
      if (post_host) post_host[(size_t)s * N + i] = cnt[i] ? P[i] : -1e30;
      if (risk_host) risk_host[(size_t)s * N + i] = cnt[i] ? R[i] : -1e30;
    }
    // by expected errors, ascending; a tie goes to the larger z, then to the smaller rank; then the others, in rank order
    std::stable_sort(ord.begin(), ord.begin() + nc, [&](int x, int y) { return R[x] != R[y] ? R[x] < R[y] : z[x] > z[y]; });
    for (int i = 0; i < N; ++i)
      if (!cnt[i]) ord[nc++] = i;
    if (order_host) std::copy(ord.begin(), ord.end(), order_host + (size_t)s * N);
  }
  mbr_t[2] += seconds_since(t1);
}

void Ctc::mbr_times(float* out3) {
  for (int i = 0; i < 3; ++i) out3[i] = (float)mbr_t[i];
  if (mbr_accumulate) mbr_t[0] = mbr_t[1] = mbr_t[2] = 0;
}

void Ctc::get_decode_candidates(int* ids_host, float* scores_host, float* blank_host, int* Cc) {
  EESEN_REQUIRE(dec.rows > 0, EESEN_ERR_STATE, "no DecodeParallel yet");
  EESEN_HIP_CHECK(hipSetDevice(device));
  EESEN_HIP_CHECK(hipStreamSynchronize(st));
  if (Cc) *Cc = dec.C;
  if (ids_host) EESEN_HIP_CHECK(hipMemcpy(ids_host, dec_i.p + dec.cid, dec.n_cand * sizeof(int), hipMemcpyDeviceToHost));
  if (scores_host) EESEN_HIP_CHECK(hipMemcpy(scores_host, dec_f.p + dec.csc, dec.n_cand * sizeof(float), hipMemcpyDeviceToHost));
  if (blank_host) EESEN_HIP_CHECK(hipMemcpy(blank_host, dec_f.p + dec.sblank, (size_t)dec.rows * sizeof(float), hipMemcpyDeviceToHost));
  for (int r = 0; r < dec.rows; ++r) {   // rows the selection never visits
    if (r / dec.S < dec_lens[r % dec.S]) continue;
    for (int c = 0; c < dec.C; ++c) {
      if (ids_host) ids_host[(size_t)r * dec.C + c] = -1;
      if (scores_host) scores_host[(size_t)r * dec.C + c] = -1e30f;
    }
    if (blank_host) blank_host[r] = -1e30f;
  }
}

void Ctc::get_alpha_beta(float* alpha_host, float* beta_host, int* Lprime) {
  EESEN_REQUIRE(last_T > 0, EESEN_ERR_STATE, "no EvalParallel yet");
  EESEN_HIP_CHECK(hipSetDevice(device));
  EESEN_HIP_CHECK(hipStreamSynchronize(st));
  const int T = last_T, S = last_S, Lpad = last_Lpad, Lp = last_Lprime;
  if (Lprime) *Lprime = Lp;
  std::vector<float> h((size_t)S * T * Lpad);
  for (int which = 0; which < 2; ++which) {
    float* dst = which == 0 ? alpha_host : beta_host;
    if (!dst) continue;
    EESEN_HIP_CHECK(hipMemcpy(h.data(), which == 0 ? alpha.p : beta.p, h.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int t = 0; t < T; ++t)
      for (int s = 0; s < S; ++s) {
        float* o = dst + ((size_t)t * S + s) * Lp;
        if (t >= last_lens[s]) {  // rows the sweep never visits; the reference leaves -1e30 there (ctc-loss.cc:138-139)
          for (int j = 0; j < Lp; ++j) o[j] = -1e30f;
        } else {
          const float* src = h.data() + ((size_t)s * T + t) * Lpad;
          for (int j = 0; j < Lp; ++j) o[j] = src[j];
        }
      }
  }
}

// LevenshteinEditDistance (src/util/edit-distance-inl.h), total errors only
static int levenshtein(const int* ref, int nr, const std::vector<int>& hyp) {
  const int nh = (int)hyp.size();
  std::vector<int> prev(nh + 1), cur(nh + 1);
  for (int j = 0; j <= nh; ++j) prev[j] = j;
  for (int i = 1; i <= nr; ++i) {
    cur[0] = i;
    for (int j = 1; j <= nh; ++j) {
      const int sub = prev[j - 1] + (ref[i - 1] == hyp[j - 1] ? 0 : 1);
      cur[j] = std::min(sub, std::min(prev[j] + 1, cur[j - 1] + 1));
    }
    std::swap(prev, cur);
  }
  return prev[nh];
}

int edit_distance(const int* ref, int nr, const int* hyp, int nh) { return levenshtein(ref, nr, std::vector<int>(hyp, hyp + nh)); }

void Ctc::flush_err(PendingErr& q, int* num_err, int* num_ref) {
  if (!q.active) return;
  q.pin.wait();
  const int* ids = q.pin.as<int>();
  const int S = q.S;
  int err = 0, ref = 0;
  if (StatGuard::raised(ids, (size_t)q.rows * sizeof(int))) {  // decoded from a timed-out forward pass (see StatGuard): not a statistic
    if (q.with_probs) q.probs.wait();
    if (num_err) *num_err = 0;
    if (num_ref) *num_ref = 0;
    q.active = false;
    return;
  }
  std::vector<int> hyp, frm;
  std::ofstream output;
  if (q.with_probs) {
    q.probs.wait();
    output.open(seq_out, std::ofstream::out | std::ofstream::app);  // ctc-loss.cc:247-250
  }
  const float* probs = q.probs.as<float>();
  for (int s = 0; s < S; ++s) {
    hyp.clear(); frm.clear();
    int last = -1;
    for (int f = 0; f < q.frames[s]; ++f) {  // collapse repeats, drop blanks (ctc-loss.cc:252-275)
      const int id = ids[(size_t)f * S + s];
      if (f == 0 || id != last) {
        if (id != 0) { hyp.push_back(id); frm.push_back(f); }
      }
      last = id;
    }
    const int U = q.off[s + 1] - q.off[s];
    err += levenshtein(q.ids.data() + q.off[s], U, hyp);
    ref += U;
    if (q.with_probs) {  // :282-291: the index of the phone, the frame, and the probability
      output << "utt";
      for (size_t i = 0; i < hyp.size(); ++i)
        output << " | " << hyp[i] << " " << frm[i] << " " << probs[((size_t)frm[i] * S + s) * q.K + hyp[i]];
      output << "\n";
    }
  }
  err_tokens += err;
  ref_tokens += ref;
  if (num_err) *num_err = err;
  if (num_ref) *num_ref = ref;
  q.active = false;
}

// With num_err == num_ref == NULL the call only ENQUEUES the argmax and the copy of the ids; collapsing and the edit
// distances (host work, ctc-loss.cc:252-296) run when the next call needs the slot or the statistics are read -- by then
// the device is busy with the backward pass, so neither side waits for the other.
void Ctc::error_rate_mseq(const int* frame_num_utt, int S, const float* net_out, int rows, int K, int ld,
                          const int* label_ids, const int* label_off, int* num_err, int* num_ref) {
  check_batch(frame_num_utt, S, rows, K, /*ld=*/K, label_ids, label_off);   // (the argmax takes any stride)
  EESEN_HIP_CHECK(hipSetDevice(device));
  if (ids_d.cap < (size_t)rows) EESEN_HIP_CHECK(hipStreamSynchronize(st));
  ids_d.reserve(rows);
  PendingErr& q = perr[perr_idx++ & 1];
  flush_err(q, nullptr, nullptr);
  row_argmax(st, net_out, ld, rows, K, ids_d.p);  // FindRowMaxId, ctc-loss.cc:238-239
  guard.read_back(q.pin, ids_d.p, (size_t)rows * sizeof(int), st);
  q.rows = rows;
  q.S = S; q.K = K; q.active = true;
  q.with_probs = !seq_out.empty();
  if (q.with_probs) {  // "This is inefficient, but ok for now" (ctc-loss.cc:283): the whole posterior matrix comes back
    float* pp = static_cast<float*>(loss_slot(q.probs, (size_t)rows * K * sizeof(float)));
    EESEN_HIP_CHECK(hipMemcpy2DAsync(pp, (size_t)K * sizeof(float), net_out, (size_t)ld * sizeof(float), (size_t)K * sizeof(float), rows,
                                     hipMemcpyDeviceToHost, st));
    q.probs.used(st);
  }
  q.frames.assign(frame_num_utt, frame_num_utt + S);
  q.off.assign(label_off, label_off + S + 1);
  for (int& o : q.off) o -= label_off[0];
  q.ids.assign(label_ids + label_off[0], label_ids + label_off[S]);
  if (num_err || num_ref) {
    flush_err(perr[perr_idx & 1], nullptr, nullptr);  // the older one first: totals accumulate in call order
    flush_err(q, num_err, num_ref);
  }
}

}  // namespace eesen
