// capi.cpp -- the extern "C" boundary declared in include/eesen_hip.h.  Every wrapper converts internal
// exceptions into a status code and a thread-local message; no exception leaves the library.
#include <cstdio>
#include <cstring>

#include <algorithm>
#include <memory>

#include "guard.h"
#include "net.h"

using namespace eesen;

#include "handles.h"

namespace eesen {
std::string& last_error_slot() {
  thread_local std::string g_err;
  return g_err;
}
}  // namespace eesen

extern "C" {

const char* eesen_last_error(void) { return last_error_slot().c_str(); }
const char* eesen_version(void) { return "eesen_hip 0.1.0 (gfx950)"; }

int eesen_device_count(int* count) {
  return guard([&] {
    REQ_PTR(count);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
  });
}

int eesen_set_gemm_mode(int mode) {
  return guard([&] {
    EESEN_REQUIRE(mode >= -1 && mode <= 2, EESEN_ERR_INVALID, "gemm mode must be -1 (environment), 0 (f32 MFMA), 1 (three bf16 planes) or 2 (two fp16 planes)");
    set_gemm_mode(mode);
  });
}
int eesen_get_gemm_mode(int* mode) {
  return guard([&] { REQ_PTR(mode); *mode = gemm_mode(); });
}

int eesen_device_synchronize(int device) {
  return guard([&] {
    EESEN_HIP_CHECK(hipSetDevice(device));
    EESEN_HIP_CHECK(hipDeviceSynchronize());
  });
}

int eesen_net_create(int device, void* stream, eesen_net_t** out) {
  return guard([&] {
    REQ_PTR(out);
    *out = new eesen_net(device, stream);
  });
}
int eesen_net_destroy(eesen_net_t* net) {
  return guard([&] { delete net; });
}
int eesen_net_add_layer(eesen_net_t* net, int kind, int in_dim, int out_dim, float coef, float max_grad) {
  return guard([&] { REQ_PTR(net); net->add_layer(kind, in_dim, out_dim, coef, max_grad); });
}
int eesen_net_set_train_mode(eesen_net_t* net, int train) {
  return guard([&] { REQ_PTR(net); net->set_train_mode(train != 0); });
}
int eesen_net_set_dropout_seed(eesen_net_t* net, unsigned long long seed) {
  return guard([&] { REQ_PTR(net); net->drop_seed = seed; net->drop_counter = 0; });
}
int eesen_net_set_layer_dropout(eesen_net_t* net, int layer, const float* nine) {
  return guard([&] { REQ_PTR(net); REQ_PTR(nine); net->set_layer_dropout(layer, nine); });
}
int eesen_net_get_layer_dropout(eesen_net_t* net, int layer, float* nine) {
  return guard([&] { REQ_PTR(net); REQ_PTR(nine); net->get_layer_dropout(layer, nine); });
}
int eesen_net_set_dropout_masks(eesen_net_t* net, int layer, const float* fwd_mask_host, long fwd_floats,
                                const float* rec_mask_host, int rec_rows, long rec_floats, int twiddle_coin) {
  return guard([&] { REQ_PTR(net); net->set_dropout_masks(layer, fwd_mask_host, fwd_floats, rec_mask_host, rec_rows, rec_floats, twiddle_coin); });
}
int eesen_net_get_dropout_masks(eesen_net_t* net, int layer, float* fwd_mask_host, float* rec_mask_host, int* info4) {
  return guard([&] { REQ_PTR(net); net->get_dropout_masks(layer, fwd_mask_host, rec_mask_host, info4); });
}
int eesen_net_finalize(eesen_net_t* net) {
  return guard([&] { REQ_PTR(net); net->finalize(); });
}
int eesen_net_read(eesen_net_t* net, const char* path) {
  return guard([&] { REQ_PTR(net); REQ_PTR(path); net->read(path); });
}
int eesen_net_write(eesen_net_t* net, const char* path, int binary) {
  return guard([&] { REQ_PTR(net); REQ_PTR(path); net->write(path, binary != 0); });
}
int eesen_net_num_layers(eesen_net_t* net, int* n) {
  return guard([&] { REQ_PTR(net); REQ_PTR(n); *n = (int)net->layers.size(); });
}
int eesen_net_layer_info(eesen_net_t* net, int idx, int* kind, int* in_dim, int* out_dim, float* coef, float* max_grad) {
  return guard([&] {
    REQ_PTR(net);
    EESEN_REQUIRE(idx >= 0 && idx < (int)net->layers.size(), EESEN_ERR_INVALID, "layer index out of range");
    const Layer& L = net->layers[idx];
    if (kind) *kind = L.kind;
    if (in_dim) *in_dim = L.din_f;     // the model's own dimensions (an LSTM layer the library pads to a multiple of 4 cells reports what the file says)
    if (out_dim) *out_dim = L.dout_f;
    if (coef) *coef = L.coef;
    if (max_grad) *max_grad = L.max_grad;
  });
}
int eesen_net_layer_marker(eesen_net_t* net, int idx, char* buf, int cap) {
  return guard([&] {
    REQ_PTR(net); REQ_PTR(buf);
    EESEN_REQUIRE(idx >= 0 && idx < (int)net->layers.size() && cap > 0, EESEN_ERR_INVALID, "layer index out of range");
    std::snprintf(buf, (size_t)cap, "%s", net->layers[idx].marker());
  });
}
int eesen_net_tensor_moments(eesen_net_t* net, int which, int layer, double* out6_host, int cap_tensors, int* n_tensors) {
  return guard([&] {
    REQ_PTR(net); REQ_PTR(n_tensors);
    *n_tensors = net->tensor_moments(which, layer, out6_host, cap_tensors);
  });
}
int eesen_net_input_dim(eesen_net_t* net, int* dim) {
  return guard([&] { REQ_PTR(net); REQ_PTR(dim); EESEN_REQUIRE(!net->layers.empty(), EESEN_ERR_STATE, "empty net"); *dim = net->layers.front().din_f; });
}
int eesen_net_output_dim(eesen_net_t* net, int* dim) {
  return guard([&] { REQ_PTR(net); REQ_PTR(dim); EESEN_REQUIRE(!net->layers.empty(), EESEN_ERR_STATE, "empty net"); *dim = net->layers.back().dout_f; });
}
int eesen_net_num_params(eesen_net_t* net, long* n) {
  return guard([&] { REQ_PTR(net); REQ_PTR(n); *n = net->num_params(); });
}
int eesen_net_get_params(eesen_net_t* net, float* host_flat, long n) {
  return guard([&] { REQ_PTR(net); REQ_PTR(host_flat); net->get_flat(net->params, host_flat, n); });
}
int eesen_net_set_params(eesen_net_t* net, const float* host_flat, long n) {
  return guard([&] { REQ_PTR(net); REQ_PTR(host_flat); net->set_params(host_flat, n); });
}
int eesen_net_set_train_options(eesen_net_t* net, float learn_rate, float momentum) {
  return guard([&] { REQ_PTR(net); net->lr = learn_rate; net->mmt = momentum; });
}
int eesen_net_set_update_algorithm(eesen_net_t* net, const char* name) {
  return guard([&] {
    REQ_PTR(net); REQ_PTR(name);
    const std::string a(name);  // Net::SetUpdateAlgorithm, net.cc:481-497
    if (a == "SGD") net->rule = 0;
    else if (a == "Adagrad") net->rule = 1;
    else if (a == "RMSProp") net->rule = 2;
    else throw Error(EESEN_ERR_INVALID, "unknown optimization algorithm '" + a + "' (SGD|Adagrad|RMSProp)");
  });
}
int eesen_net_set_adaptive_options(eesen_net_t* net, float adagrad_epsilon, float rmsprop_rho) {
  return guard([&] { REQ_PTR(net); net->ada_eps = adagrad_epsilon; net->rms_rho = rmsprop_rho; net->rms_one_minus_rho = 1.0f - rmsprop_rho; });
}
int eesen_net_get_accumulators(eesen_net_t* net, float* host_flat, long n) {
  return guard([&] { REQ_PTR(net); REQ_PTR(host_flat); net->init_accu(); net->get_flat(net->accu, host_flat, n); });
}
int eesen_net_set_accumulators(eesen_net_t* net, const float* host_flat, long n) {
  return guard([&] { REQ_PTR(net); REQ_PTR(host_flat); net->set_accu(host_flat, n); });
}
int eesen_net_set_seq_lengths(eesen_net_t* net, const int* lens, int S) {
  return guard([&] { REQ_PTR(net); REQ_PTR(lens); net->set_seq_lengths(lens, S); });
}
int eesen_net_propagate(eesen_net_t* net, const float* in, int rows, int in_ld, int in_is_device, const float** out_dev,
                        int* out_cols, int* out_ld) {
  return guard([&] {
    REQ_PTR(net); REQ_PTR(in);
    net->propagate(in, rows, in_ld, in_is_device != 0);
    if (out_dev) *out_dev = net->out_ptr;
    if (out_cols) *out_cols = net->out_cols;
    if (out_ld) *out_ld = net->out_ld;
  });
}
int eesen_net_get_output(eesen_net_t* net, float* host_out, long n) {
  return guard([&] {
    REQ_PTR(net); REQ_PTR(host_out);
    EESEN_REQUIRE(net->propagated, EESEN_ERR_STATE, "no Propagate output");
    EESEN_REQUIRE(n == (long)net->rows * net->out_cols, EESEN_ERR_INVALID, "output size mismatch");
    net->sync();
    EESEN_HIP_CHECK(hipMemcpy2D(host_out, (size_t)net->out_cols * 4, net->out_ptr, (size_t)net->out_ld * 4, (size_t)net->out_cols * 4,
                                net->rows, hipMemcpyDeviceToHost));
  });
}
int eesen_net_backpropagate(eesen_net_t* net, const float* out_diff_dev, int out_diff_ld, float* in_diff_dev, int in_diff_ld) {
  return guard([&] { REQ_PTR(net); REQ_PTR(out_diff_dev); net->backpropagate(out_diff_dev, out_diff_ld, in_diff_dev, in_diff_ld); });
}
int eesen_net_grad_buffer(eesen_net_t* net, float** dev_ptr, long* n) {
  return guard([&] { REQ_PTR(net); REQ_PTR(dev_ptr); REQ_PTR(n); *dev_ptr = net->fresh.p; *n = (long)net->P; });
}
int eesen_net_get_grads(eesen_net_t* net, float* host_flat, long n) {
  return guard([&] { REQ_PTR(net); REQ_PTR(host_flat); net->get_flat(net->fresh, host_flat, n); });
}
int eesen_net_update(eesen_net_t* net) {
  return guard([&] { REQ_PTR(net); net->update(); });
}
int eesen_net_set_forward_precision(eesen_net_t* net, int bf16) {
  return guard([&] { REQ_PTR(net); net->fwd_bf16 = bf16 != 0; net->fwd_bf16_rec = bf16 == 1; });
}
int eesen_net_bf16_recurrence_layers(eesen_net_t* net, int* layers) {
  return guard([&] { REQ_PTR(net); REQ_PTR(layers); *layers = net->info_fwd_bf16; });
}
int eesen_net_plan_string(eesen_net_t* net, char* json, int cap) {
  return guard([&] {
    REQ_PTR(net); REQ_PTR(json);
    const std::string s = net->plan_string();
    EESEN_REQUIRE(cap > (int)s.size(), EESEN_ERR_INVALID, "eesen_net_plan_string: buffer too small (" + std::to_string(s.size() + 1) + " bytes needed)");
    std::memcpy(json, s.c_str(), s.size() + 1);
  });
}
int eesen_net_recurrence_info(eesen_net_t* net, int* out3) {  // four ints
  return guard([&] {
    REQ_PTR(net); REQ_PTR(out3);
    out3[0] = net->info_lstm_layers; out3[1] = net->info_fwd_persistent; out3[2] = net->info_bwd_persistent;
    out3[3] = net->recoveries;
  });
}
int eesen_net_debug_set_error_word(eesen_net_t* net, unsigned value) {
  return guard([&] {
    REQ_PTR(net);
    EESEN_HIP_CHECK(hipSetDevice(net->device));
    EESEN_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(net->ctl.p + kCtlWords - 1), (int)value, 1, net->st));
  });
}
int eesen_net_debug_layer_buffer(eesen_net_t* net, int layer, int which, float* host, long cap_floats, int* rows, int* cols) {
  return guard([&] { REQ_PTR(net); net->debug_layer_buffer(layer, which, host, cap_floats, rows, cols); });
}
int eesen_net_synchronize(eesen_net_t* net) {
  return guard([&] { REQ_PTR(net); net->sync(); });
}
int eesen_net_set_profiling(eesen_net_t* net, int on) {
  return guard([&] { REQ_PTR(net); net->timer.enable(on != 0); net->timer.set_accumulate(on == 2); });
}
int eesen_net_get_phase_spans(eesen_net_t* net, int* phases, float* seconds, int cap, int* n) {
  return guard([&] { REQ_PTR(net); REQ_PTR(n); *n = net->timer.spans(phases, seconds, cap); });
}
int eesen_net_get_phase_times(eesen_net_t* net, float* out6) {
  return guard([&] { REQ_PTR(net); REQ_PTR(out6); net->timer.collect(out6, 6); });
}

int eesen_ctc_create(int device, void* stream, eesen_ctc_t** out) {
  return guard([&] { REQ_PTR(out); *out = new eesen_ctc(device, stream); });
}
int eesen_ctc_destroy(eesen_ctc_t* ctc) {
  return guard([&] { delete ctc; });
}
int eesen_ctc_eval_parallel(eesen_ctc_t* ctc, const int* frame_num_utt, int S, const float* net_out_dev, int rows, int K,
                            int ld, const int* label_ids, const int* label_off, float* diff_dev, int diff_ld,
                            float* pzx_host) {
  return guard([&] {
    REQ_PTR(ctc); REQ_PTR(frame_num_utt); REQ_PTR(net_out_dev); REQ_PTR(label_ids); REQ_PTR(label_off); REQ_PTR(diff_dev);
    ctc->eval_parallel(frame_num_utt, S, net_out_dev, rows, K, ld, label_ids, label_off, diff_dev, diff_ld, pzx_host);
  });
}
int eesen_ctc_align_parallel(eesen_ctc_t* ctc, const int* frame_num_utt, int S, const float* scores_dev, int rows, int K, int ld,
                             int is_log, const int* label_ids, const int* label_off, int* ali_host, int* pos_host, float* score_host) {
  return guard([&] {
    REQ_PTR(ctc); REQ_PTR(frame_num_utt); REQ_PTR(scores_dev); REQ_PTR(label_ids); REQ_PTR(label_off); REQ_PTR(ali_host); REQ_PTR(score_host);
    ctc->align_parallel(frame_num_utt, S, scores_dev, rows, K, ld, is_log != 0, label_ids, label_off, ali_host, pos_host, score_host);
  });
}
int eesen_ctc_get_align_times(eesen_ctc_t* ctc, float* out3) {
  return guard([&] { REQ_PTR(ctc); REQ_PTR(out3); ctc->align_times(out3); });
}
int eesen_ctc_decode_parallel(eesen_ctc_t* ctc, const int* frame_num_utt, int S, const float* scores_dev, int rows, int K, int ld,
                              int is_log, int beam, int max_classes, int nbest, int* hyp_host, int* hyp_len_host, float* score_host) {
  return guard([&] {
    REQ_PTR(ctc); REQ_PTR(frame_num_utt); REQ_PTR(scores_dev); REQ_PTR(hyp_host); REQ_PTR(hyp_len_host); REQ_PTR(score_host);
    ctc->decode_parallel(frame_num_utt, S, scores_dev, rows, K, ld, is_log != 0, beam, max_classes, nbest, hyp_host, hyp_len_host, score_host);
  });
}
int eesen_ctc_get_decode_times(eesen_ctc_t* ctc, float* out3) {
  return guard([&] { REQ_PTR(ctc); REQ_PTR(out3); ctc->decode_times(out3); });
}
int eesen_ctc_get_decode_candidates(eesen_ctc_t* ctc, int* ids_host, float* scores_host, float* blank_host, int* num_classes) {
  return guard([&] { REQ_PTR(ctc); ctc->get_decode_candidates(ids_host, scores_host, blank_host, num_classes); });
}
int eesen_lm_create_from_arpa(const char* arpa_path, const char* units_path, int K, eesen_lm_t** lm) {
  return guard([&] {
    REQ_PTR(arpa_path); REQ_PTR(lm);
    std::unique_ptr<eesen_lm> made(new eesen_lm);
    made->from_arpa(arpa_path, units_path, K);
    *lm = made.release();
  });
}
int eesen_lm_create_from_arpa_ex(const char* arpa_path, const char* units_path, int K, int skip_oov, eesen_lm_t** lm) {
  return guard([&] {
    REQ_PTR(arpa_path); REQ_PTR(lm);
    std::unique_ptr<eesen_lm> made(new eesen_lm);
    made->from_arpa(arpa_path, units_path, K, skip_oov != 0);
    *lm = made.release();
  });
}
int eesen_lm_oov_dropped(eesen_lm_t* lm, long long* ngrams) {
  return guard([&] { REQ_PTR(lm); REQ_PTR(ngrams); *ngrams = lm->oov_dropped; });
}
int eesen_lm_destroy(eesen_lm_t* lm) {
  return guard([&] { delete lm; });
}
int eesen_lm_info(eesen_lm_t* lm, int* order, int* states, int* arcs, int* has_eos) {
  return guard([&] {
    REQ_PTR(lm);
    if (order) *order = lm->order;
    if (states) *states = lm->states();
    if (arcs) *arcs = lm->arcs();
    if (has_eos) *has_eos = lm->has_eos ? 1 : 0;
  });
}
int eesen_lm_step(eesen_lm_t* lm, int state, int c, float* w, int* next) {
  return guard([&] { REQ_PTR(lm); REQ_PTR(w); REQ_PTR(next); lm->step(state, c, w, next); });
}
int eesen_lm_start(eesen_lm_t* lm, int* state) {
  return guard([&] { REQ_PTR(lm); REQ_PTR(state); *state = lm->start; });
}
int eesen_lm_final(eesen_lm_t* lm, int state, float* w) {
  return guard([&] {
    REQ_PTR(lm); REQ_PTR(w);
    EESEN_REQUIRE(state >= 0 && state < lm->states(), EESEN_ERR_INVALID, "LM state out of range");
    *w = lm->fin[state];
  });
}
int eesen_lm_score(eesen_lm_t* lm, const int* labels, int n, int use_eos, double* logprob_f64, double* abs_sum_f64) {
  return guard([&] {
    REQ_PTR(lm); REQ_PTR(logprob_f64);
    EESEN_REQUIRE(n >= 0 && (n == 0 || labels != nullptr), EESEN_ERR_INVALID, "labels: null pointer or negative count");
    *logprob_f64 = lm->score(labels, n, use_eos != 0, abs_sum_f64);
  });
}
int eesen_lex_create(const char* lexicon_path, const char* units_path, int K, int space_class, eesen_lex_t** lex) {
  return guard([&] {
    REQ_PTR(lexicon_path); REQ_PTR(lex);
    std::unique_ptr<eesen_lex> made(new eesen_lex);
    made->from_file(lexicon_path, units_path, K, space_class);
    *lex = made.release();
  });
}
int eesen_lex_destroy(eesen_lex_t* lex) {
  return guard([&] { delete lex; });
}
int eesen_lex_info(eesen_lex_t* lex, int* words, int* nodes, int* max_word_len) {
  return guard([&] {
    REQ_PTR(lex);
    if (words) *words = lex->V();
    if (nodes) *nodes = lex->nodes();
    if (max_word_len) *max_word_len = lex->max_word_len;
  });
}
int eesen_lex_write_words(eesen_lex_t* lex, const char* path) {
  return guard([&] { REQ_PTR(lex); REQ_PTR(path); lex->write_words(path); });
}
int eesen_lex_child(eesen_lex_t* lex, int node, int c, int* child) {
  return guard([&] { REQ_PTR(lex); REQ_PTR(child); *child = lex->child(node, c); });
}
int eesen_lex_word(eesen_lex_t* lex, int node, int* word) {
  return guard([&] {
    REQ_PTR(lex); REQ_PTR(word);
    EESEN_REQUIRE(node >= 0 && node < lex->nodes(), EESEN_ERR_INVALID, "lexicon node out of range");
    *word = lex->word[node];
  });
}
int eesen_lex_words(eesen_lex_t* lex, const int* labels, int n, int* words_out, int* num_words) {
  return guard([&] {
    REQ_PTR(lex); REQ_PTR(num_words);
    EESEN_REQUIRE(n >= 0 && (n == 0 || (labels != nullptr && words_out != nullptr)), EESEN_ERR_INVALID, "labels / words_out: null pointer or negative count");
    EESEN_REQUIRE(lex->words(labels, n, words_out, num_words), EESEN_ERR_INVALID, "the labelling is no sequence of lexicon words separated by single spaces");
  });
}
int eesen_ctc_decode_parallel_lex(eesen_ctc_t* ctc, const int* frame_num_utt, int S, const float* scores_dev, int rows, int K, int ld,
                                  int is_log, int beam, int max_classes, int nbest, eesen_lex_t* lex, eesen_lm_t* lm, float lm_weight,
                                  float word_bonus, int use_eos, int* hyp_host, int* hyp_len_host, float* score_host, float* lm_score_host,
                                  int* word_host, int* word_len_host) {
  return guard([&] {
    REQ_PTR(ctc); REQ_PTR(frame_num_utt); REQ_PTR(scores_dev); REQ_PTR(hyp_host); REQ_PTR(hyp_len_host); REQ_PTR(score_host);
    ctc->decode_parallel_lex(frame_num_utt, S, scores_dev, rows, K, ld, is_log != 0, beam, max_classes, nbest, lex, lm, lm_weight, word_bonus,
                             use_eos != 0, hyp_host, hyp_len_host, score_host, lm_score_host, word_host, word_len_host);
  });
}
int eesen_lex_create_unspaced(const char* lexicon_path, const char* units_path, int K, eesen_lex_t** lex) {
  return guard([&] {
    REQ_PTR(lexicon_path); REQ_PTR(lex);
    std::unique_ptr<eesen_lex> made(new eesen_lex);
    made->from_file_unspaced(lexicon_path, units_path, K);
    *lex = made.release();
  });
}
int eesen_lex_max_homophones(eesen_lex_t* lex, int* H) {
  return guard([&] { REQ_PTR(lex); REQ_PTR(H); *H = lex->max_homophones; });
}
int eesen_lex_node_words(eesen_lex_t* lex, int node, int* out, int cap, int* count) {
  return guard([&] {
    REQ_PTR(lex); REQ_PTR(count);
    EESEN_REQUIRE(node >= 0 && node < lex->nodes(), EESEN_ERR_INVALID, "lexicon node out of range");
    EESEN_REQUIRE(cap >= 0 && (cap == 0 || out != nullptr), EESEN_ERR_INVALID, "out: null pointer or negative capacity");
    const int n = lex->unspaced ? lex->wcount[node] : (lex->word[node] != 0 ? 1 : 0);
    for (int i = 0; i < std::min(n, cap); ++i) out[i] = lex->unspaced ? lex->node_words[lex->wfirst[node] + i] : lex->word[node];
    *count = n;
  });
}
int eesen_ctc_decode_parallel_words(eesen_ctc_t* ctc, const int* frame_num_utt, int S, const float* scores_dev, int rows, int K, int ld,
                                    int is_log, int beam, int max_classes, int nbest, eesen_lex_t* lex, eesen_lm_t* lm, float lm_weight,
                                    float word_bonus, int use_eos, int* hyp_host, int* hyp_len_host, float* score_host, float* lm_score_host,
                                    int* word_host, int* word_len_host, int* word_end_host) {
  return guard([&] {
    REQ_PTR(ctc); REQ_PTR(frame_num_utt); REQ_PTR(scores_dev); REQ_PTR(hyp_host); REQ_PTR(hyp_len_host); REQ_PTR(score_host);
    ctc->decode_parallel_words(frame_num_utt, S, scores_dev, rows, K, ld, is_log != 0, beam, max_classes, nbest, lex, lm, lm_weight, word_bonus,
                               use_eos != 0, hyp_host, hyp_len_host, score_host, lm_score_host, word_host, word_len_host, word_end_host);
  });
}
int eesen_lex_lookahead(eesen_lex_t* lex, eesen_lm_t* lm, float* out_host, int cap) {
  return guard([&] {
    REQ_PTR(lex); REQ_PTR(lm); REQ_PTR(out_host);
    EESEN_REQUIRE(cap >= lex->nodes(), EESEN_ERR_INVALID, "the look-ahead table has one value per lexicon node: cap is below eesen_lex_info's node count");
    lex->lookahead(*lm, out_host);
  });
}
int eesen_ctc_set_lm_lookahead(eesen_ctc_t* ctc, int mode) {
  return guard([&] {
    REQ_PTR(ctc);
    EESEN_REQUIRE(mode == 0 || mode == 1, EESEN_ERR_INVALID, "LM look-ahead mode: 0 (off) or 1 (unigram)");
    ctc->lm_lookahead = mode;
  });
}
int eesen_ctc_get_lm_lookahead(eesen_ctc_t* ctc, int* mode) {
  return guard([&] { REQ_PTR(ctc); REQ_PTR(mode); *mode = ctc->lm_lookahead; });
}
int eesen_ctc_decode_parallel_lm(eesen_ctc_t* ctc, const int* frame_num_utt, int S, const float* scores_dev, int rows, int K, int ld,
                                 int is_log, int beam, int max_classes, int nbest, eesen_lm_t* lm, float lm_weight, float insertion_bonus,
                                 int use_eos, int* hyp_host, int* hyp_len_host, float* score_host, float* lm_score_host) {
  return guard([&] {
    REQ_PTR(ctc); REQ_PTR(frame_num_utt); REQ_PTR(scores_dev); REQ_PTR(hyp_host); REQ_PTR(hyp_len_host); REQ_PTR(score_host);
    ctc->decode_parallel_lm(frame_num_utt, S, scores_dev, rows, K, ld, is_log != 0, beam, max_classes, nbest, lm, lm_weight, insertion_bonus,
                            use_eos != 0, hyp_host, hyp_len_host, score_host, lm_score_host);
  });
}
int eesen_ctc_decode_stamps(eesen_ctc_t* ctc, const int* frame_num_utt, int S, const float* scores_dev, int rows, int K, int ld, int is_log,
                            double conf_scale, int* lstart_host, int* lend_host, int* wstart_host, int* wend_host, float* wconf_host,
                            float* path_score_host) {
  return guard([&] {
    REQ_PTR(ctc); REQ_PTR(frame_num_utt); REQ_PTR(scores_dev);
    ctc->decode_stamps(frame_num_utt, S, scores_dev, rows, K, ld, is_log != 0, conf_scale, lstart_host, lend_host, wstart_host, wend_host,
                       wconf_host, path_score_host);
  });
}
int eesen_ctc_score_parallel(eesen_ctc_t* ctc, const int* frame_num_utt, int S, const float* scores_dev, int rows, int K, int ld, int is_log,
                             const int* hyp_off, const int* label_off, const int* label_ids, float* score_host) {
  return guard([&] {
    REQ_PTR(ctc); REQ_PTR(frame_num_utt); REQ_PTR(scores_dev); REQ_PTR(hyp_off); REQ_PTR(label_off);
    EESEN_REQUIRE(S > 0, EESEN_ERR_INVALID, "rows must be a positive multiple of the sequence count");
    // (every labelling may be empty: then there is no label to point to)
    EESEN_REQUIRE(label_ids != nullptr || hyp_off[S] <= 0 || label_off[hyp_off[S]] == label_off[0], EESEN_ERR_INVALID, "label_ids is null");
    ctc->score_parallel(frame_num_utt, S, scores_dev, rows, K, ld, is_log != 0, hyp_off, label_off, label_ids, score_host);
  });
}
int eesen_ctc_decode_rescore(eesen_ctc_t* ctc, const int* frame_num_utt, int S, const float* scores_dev, int rows, int K, int ld, int is_log,
                             eesen_lm_t* lm, float lm_weight, float bonus, int use_eos, float* am_score_host, float* lm_score_host,
                             float* total_host, int* order_host) {
  return guard([&] {
    REQ_PTR(ctc); REQ_PTR(frame_num_utt); REQ_PTR(scores_dev);
    ctc->decode_rescore(frame_num_utt, S, scores_dev, rows, K, ld, is_log != 0, lm, lm_weight, bonus, use_eos != 0, am_score_host,
                        lm_score_host, total_host, order_host);
  });
}
int eesen_ctc_get_rescore_times(eesen_ctc_t* ctc, float* out3) {
  return guard([&] { REQ_PTR(ctc); REQ_PTR(out3); ctc->rescore_times(out3); });
}
int eesen_edit_distance_parallel(eesen_ctc_t* ctc, int G, const int* seq_off, const int* tok_off, const int* tok_ids, const int* ref_off,
                                 const int* ref_ids, int* pair_host, int* ref_dist_host) {
  return guard([&] {
    REQ_PTR(ctc);
    EESEN_REQUIRE(G >= 0, EESEN_ERR_INVALID, "edit distances: negative group count");
    if (G == 0) return;
    REQ_PTR(seq_off); REQ_PTR(tok_off);
    ctc->edit_distance_parallel(G, seq_off, tok_off, tok_ids, ref_off, ref_ids, pair_host, ref_dist_host);
  });
}
int eesen_ctc_decode_mbr(eesen_ctc_t* ctc, int S, int level, double scale, const float* total_host, const int* ref_off, const int* ref_ids,
                         int* dist_host, int* ref_dist_host, double* post_host, double* risk_host, int* order_host) {
  return guard([&] {
    REQ_PTR(ctc);
    ctc->decode_mbr(S, level, scale, total_host, ref_off, ref_ids, dist_host, ref_dist_host, post_host, risk_host, order_host);
  });
}
int eesen_ctc_get_mbr_times(eesen_ctc_t* ctc, float* out3) {
  return guard([&] { REQ_PTR(ctc); REQ_PTR(out3); ctc->mbr_times(out3); });
}
int eesen_ctc_get_stamp_times(eesen_ctc_t* ctc, float* out3) {
  return guard([&] { REQ_PTR(ctc); REQ_PTR(out3); ctc->stamp_times(out3); });
}
int eesen_ctc_set_stamp_group(eesen_ctc_t* ctc, int lattices) {
  return guard([&] {
    REQ_PTR(ctc);
    EESEN_REQUIRE(lattices >= 0, EESEN_ERR_INVALID, "stamp group: a negative lattice count");
    ctc->stamp_group = lattices;
  });
}
int eesen_word_confidence(int n_entries, const double* scores, const int* word_len, const int* word_ids, const int* wstart, const int* wend,
                          int stride, double conf_scale, double* conf_out) {
  return guard([&] {
    REQ_PTR(scores); REQ_PTR(word_len); REQ_PTR(word_ids); REQ_PTR(wstart); REQ_PTR(wend); REQ_PTR(conf_out);
    word_confidence(n_entries, scores, word_len, word_ids, wstart, wend, stride, conf_scale, conf_out);
  });
}
int eesen_edit_distance(const int* ref, int num_ref, const int* hyp, int num_hyp, int* errors) {
  return guard([&] {
    REQ_PTR(errors);
    if (num_ref < 0 || num_hyp < 0 || (num_ref > 0 && !ref) || (num_hyp > 0 && !hyp)) throw Error(EESEN_ERR_INVALID, "edit distance: bad sequence");
    *errors = edit_distance(ref, num_ref, hyp, num_hyp);
  });
}
int eesen_ctc_error_rate_mseq(eesen_ctc_t* ctc, const int* frame_num_utt, int S, const float* net_out_dev, int rows, int K,
                              int ld, const int* label_ids, const int* label_off, int* num_err, int* num_ref) {
  return guard([&] {
    REQ_PTR(ctc); REQ_PTR(frame_num_utt); REQ_PTR(net_out_dev); REQ_PTR(label_ids); REQ_PTR(label_off);
    ctc->error_rate_mseq(frame_num_utt, S, net_out_dev, rows, K, ld, label_ids, label_off, num_err, num_ref);
  });
}
int eesen_ctc_stats(eesen_ctc_t* ctc, double* obj_sum, long* sequences, long* frames, long* err_tokens, long* ref_tokens) {
  return guard([&] {
    REQ_PTR(ctc);
    ctc->flush();  // deferred results of earlier calls
    if (obj_sum) *obj_sum = ctc->obj_sum;
    if (sequences) *sequences = ctc->sequences;
    if (frames) *frames = ctc->frames;
    if (err_tokens) *err_tokens = ctc->err_tokens;
    if (ref_tokens) *ref_tokens = ctc->ref_tokens;
  });
}
int eesen_ctc_get_alpha_beta(eesen_ctc_t* ctc, float* alpha_host, float* beta_host, int* Lprime) {
  return guard([&] { REQ_PTR(ctc); ctc->get_alpha_beta(alpha_host, beta_host, Lprime); });
}
int eesen_ctc_set_sequence_out_file(eesen_ctc_t* ctc, const char* path) {
  return guard([&] {
    REQ_PTR(ctc);
    ctc->flush();
    ctc->seq_out = path ? path : "";
    if (!ctc->seq_out.empty()) std::remove(ctc->seq_out.c_str());  // train-ctc-parallel.cc:134-137
  });
}
int eesen_ctc_set_guard(eesen_ctc_t* ctc, eesen_net_t* net) {
  return guard([&] {
    REQ_PTR(ctc);
    ctc->flush();
    ctc->guard.hook(net, ctc->device, ctc->st, "eesen_ctc_set_guard");
  });
}
int eesen_ctc_dropped(eesen_ctc_t* ctc, long* minibatches) {
  return guard([&] { REQ_PTR(ctc); REQ_PTR(minibatches); ctc->flush(); *minibatches = ctc->guard.dropped; });
}
int eesen_ctc_set_profiling(eesen_ctc_t* ctc, int mode) {
  return guard([&] { REQ_PTR(ctc); ctc->set_profiling(mode); });
}
int eesen_ctc_get_phase_times(eesen_ctc_t* ctc, float* out3) {
  return guard([&] { REQ_PTR(ctc); REQ_PTR(out3); ctc->phase_times(out3); });
}

int eesen_ce_create(int device, void* stream, eesen_ce_t** out) {
  return guard([&] { REQ_PTR(out); *out = new eesen_ce(device, stream); });
}
int eesen_ce_destroy(eesen_ce_t* ce) {
  return guard([&] { delete ce; });
}
int eesen_ce_eval_parallel(eesen_ce_t* ce, const int* frame_num_utt, int S, const float* net_out_dev, int rows, int K, int ld,
                           const int* targets_host, float* diff_dev, int diff_ld, double* obj_host) {
  return guard([&] {
    REQ_PTR(ce); REQ_PTR(frame_num_utt); REQ_PTR(net_out_dev); REQ_PTR(targets_host); REQ_PTR(diff_dev);
    ce->eval_parallel(frame_num_utt, S, net_out_dev, rows, K, ld, targets_host, diff_dev, diff_ld, obj_host);
  });
}
int eesen_ce_set_report_step(eesen_ce_t* ce, int report_step) {
  return guard([&] { REQ_PTR(ce); ce->flush(); ce->report_step = report_step; });
}
int eesen_ce_stats(eesen_ce_t* ce, double* obj, long* correct, long* frames, long* sequences) {
  return guard([&] {
    REQ_PTR(ce);
    ce->flush();
    if (obj) *obj = ce->obj;
    if (correct) *correct = ce->correct;
    if (frames) *frames = ce->frames;
    if (sequences) *sequences = ce->sequences;
  });
}
int eesen_ce_report(eesen_ce_t* ce, char* buf, int cap) {
  return guard([&] {
    REQ_PTR(ce); REQ_PTR(buf);
    const std::string s = ce->report();
    EESEN_REQUIRE(cap > (int)s.size(), EESEN_ERR_INVALID, "eesen_ce_report: buffer too small (" + std::to_string(s.size() + 1) + " bytes needed)");
    std::memcpy(buf, s.c_str(), s.size() + 1);
  });
}
int eesen_ce_progress(eesen_ce_t* ce, int wait, char* buf, int cap) {
  return guard([&] {
    REQ_PTR(ce); REQ_PTR(buf);
    EESEN_REQUIRE(cap > 0, EESEN_ERR_INVALID, "eesen_ce_progress: no buffer");
    if (wait) ce->flush();
    if (ce->progress.empty()) { buf[0] = 0; return; }
    const std::string& s = ce->progress.front();
    EESEN_REQUIRE(cap > (int)s.size(), EESEN_ERR_INVALID, "eesen_ce_progress: buffer too small (" + std::to_string(s.size() + 1) + " bytes needed)");
    std::memcpy(buf, s.c_str(), s.size() + 1);
    ce->progress.erase(ce->progress.begin());
  });
}
int eesen_ce_set_guard(eesen_ce_t* ce, eesen_net_t* net) {
  return guard([&] {
    REQ_PTR(ce);
    ce->flush();
    ce->guard.hook(net, ce->device, ce->st, "eesen_ce_set_guard");
  });
}
int eesen_ce_dropped(eesen_ce_t* ce, long* minibatches) {
  return guard([&] { REQ_PTR(ce); REQ_PTR(minibatches); ce->flush(); *minibatches = ce->guard.dropped; });
}
int eesen_ce_set_profiling(eesen_ce_t* ce, int mode) {
  return guard([&] { REQ_PTR(ce); ce->clock.set_mode(mode == 2); });
}
int eesen_ce_get_phase_times(eesen_ce_t* ce, float* out1) {
  return guard([&] { REQ_PTR(ce); REQ_PTR(out1); ce->phase_times(out1); });
}

int eesen_dev_alloc(int device, long bytes, void** dev_ptr) {
  return guard([&] {
    REQ_PTR(dev_ptr);
    EESEN_HIP_CHECK(hipSetDevice(device));
    EESEN_HIP_CHECK(hipMalloc(dev_ptr, (size_t)bytes));
  });
}
int eesen_dev_free(int device, void* dev_ptr) {
  return guard([&] {
    EESEN_HIP_CHECK(hipSetDevice(device));
    EESEN_HIP_CHECK(hipFree(dev_ptr));
  });
}
int eesen_dev_copy(int device, void* dst, const void* src, long bytes, int kind) {
  return guard([&] {
    EESEN_HIP_CHECK(hipSetDevice(device));
    const hipMemcpyKind k = kind == 1 ? hipMemcpyHostToDevice : kind == 2 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    EESEN_HIP_CHECK(hipMemcpy(dst, src, (size_t)bytes, k));
  });
}

int eesen_op_gemm(int device, void* stream, int a_kc, int b_kc, int M, int N, int K, float alpha, const float* A, int lda,
                  const float* B, int ldb, float beta, float* C, int ldc, const float* bias) {
  return guard([&] {
    EESEN_HIP_CHECK(hipSetDevice(device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // private split-K workspace for this standalone call
    DevBuf<float> ws;
    ws.reserve((size_t)8 << 20);
    gemm_f32(st, a_kc != 0, b_kc != 0, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, bias, ws.p, ws.cap);
    EESEN_HIP_CHECK(hipStreamSynchronize(st));
  });
}

int eesen_op_gemm_async(int device, void* stream, int a_kc, int b_kc, int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                        float* C, int ldc, float* ws, long ws_floats, int extra_lds_bytes) {
  return guard([&] {
    REQ_PTR(A); REQ_PTR(B); REQ_PTR(C);
    EESEN_REQUIRE(ws_floats >= 0 && (ws || ws_floats == 0) && extra_lds_bytes >= 0, EESEN_ERR_INVALID, "bad workspace / LDS cap");
    EESEN_HIP_CHECK(hipSetDevice(device));
    gemm_f32(reinterpret_cast<hipStream_t>(stream), a_kc != 0, b_kc != 0, M, N, K, 1.f, A, lda, B, ldb, 0.f, C, ldc, nullptr, ws, (size_t)ws_floats,
             extra_lds_bytes);
  });
}

int eesen_op_log_sub_prior(int device, void* stream, float* m_dev, int rows, int cols, int ld, int apply_log,
                           const float* log_priors_host, float prior_scale) {
  return guard([&] {
    REQ_PTR(m_dev);
    EESEN_HIP_CHECK(hipSetDevice(device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DevBuf<float> pri;
    if (log_priors_host) {
      pri.reserve(cols);
      EESEN_HIP_CHECK(hipMemcpyAsync(pri.p, log_priors_host, sizeof(float) * cols, hipMemcpyHostToDevice, st));
    }
    log_sub_prior(st, m_dev, ld, rows, cols, apply_log != 0, log_priors_host ? pri.p : nullptr, prior_scale);
    EESEN_HIP_CHECK(hipStreamSynchronize(st));
  });
}

int eesen_op_gemm_bench(int device, int a_kc, int b_kc, int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                        float* C, int ldc, int iters, float* avg_ms) {
  return guard([&] {
    REQ_PTR(avg_ms);
    EESEN_HIP_CHECK(hipSetDevice(device));
    DevBuf<float> ws;
    ws.reserve((size_t)16 << 20);
    DevEvent e0(true), e1(true);
    // the operand bounds of the two-plane mode are measured once, outside the timed loop (the Net keeps them per tensor)
    DevBuf<float> am;
    am.reserve((size_t)M + N + (size_t)kAmaxBlocks * 16384);
    GemmBound ba{am.p, 1}, bb{am.p + M, 1};
    float* aws = am.p + M + N;
    if (a_kc) amax_rows_cols(nullptr, A, M, K, lda, am.p, nullptr, nullptr); else amax_rows_cols(nullptr, A, K, M, lda, nullptr, am.p, aws);
    if (b_kc) amax_rows_cols(nullptr, B, N, K, ldb, am.p + M, nullptr, nullptr); else amax_rows_cols(nullptr, B, K, N, ldb, nullptr, am.p + M, aws);
    for (int i = 0; i < 2; ++i) gemm_f32(nullptr, a_kc != 0, b_kc != 0, M, N, K, 1.f, A, lda, B, ldb, 0.f, C, ldc, nullptr, ws.p, ws.cap, 0, false, ba, bb);
    e0.record(nullptr);
    for (int i = 0; i < iters; ++i) gemm_f32(nullptr, a_kc != 0, b_kc != 0, M, N, K, 1.f, A, lda, B, ldb, 0.f, C, ldc, nullptr, ws.p, ws.cap, 0, false, ba, bb);
    e1.record(nullptr);
    e1.wait();
    float ms = 0.f;
    EESEN_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    *avg_ms = ms / iters;
  });
}

int eesen_op_amax_rows_cols(int device, const float* m_dev, long rows, int cols, int ld, float* out_rows_dev, float* out_cols_dev) {
  return guard([&] {
    REQ_PTR(m_dev);
    EESEN_REQUIRE(rows > 0 && cols > 0 && ld >= cols, EESEN_ERR_INVALID, "bad matrix shape");
    EESEN_HIP_CHECK(hipSetDevice(device));
    DevBuf<float> ws;
    if (out_cols_dev) ws.reserve((size_t)kAmaxBlocks * 16384);
    amax_rows_cols(nullptr, m_dev, rows, cols, ld, out_rows_dev, out_cols_dev, ws.p);
    EESEN_HIP_CHECK(hipStreamSynchronize(nullptr));
  });
}

}  // extern "C"
