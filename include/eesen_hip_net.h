/* eesen_hip_net.h -- the C++ seam: eesen::Net / eesen::Ctc / eesen::CE / eesen::CuMatrix over the C-ABI of eesen_hip.h.
 *
 * With this header (and the four one-line forwarding headers of include/eesen_seam/, which shadow net/net.h,
 * net/ctc-loss.h, net/communicator.h and gpucompute/cuda-device.h on the include path) the reference's OWN trainer,
 * /root/reference/src/netbin/train-ctc-parallel.cc, compiles UNMODIFIED against libeesen_hip.so:
 *
 *   g++ -std=c++11 -I<repo>/include/eesen_seam -I<repo>/include -I<eesen>/src ... <eesen>/src/netbin/train-ctc-parallel.cc \
 *       <eesen base/util/cpucompute objects> -L<repo>/eesen_amd/lib -leesen_hip
 *
 * (oracle/ref_build/Makefile target `seam` does exactly that; tests/test_gpu_cli.py checks that the resulting binary and
 * eesen_amd/bin/train-ctc-parallel write byte-identical models.)  The reference's base / util / cpucompute layers (logging,
 * ParseOptions, Kaldi tables, the host Matrix) stay the reference's; everything below eesen::Net / eesen::Ctc --
 * src/net/{net,layer,*-layer,ctc-loss}, src/gpucompute -- is replaced.
 *
 * Each class states the reference interface it stands in for.  Only what train-ctc-parallel.cc (and net-output-extract.cc)
 * call is provided.  Errors: KALDI_ERR semantics, i.e. std::runtime_error carrying eesen_last_error().
 */
#ifndef EESEN_HIP_NET_H_
#define EESEN_HIP_NET_H_

#include <cstdlib>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "base/kaldi-common.h"     /* the reference's: int32, BaseFloat, KALDI_LOG / KALDI_ERR */
#include "cpucompute/matrix.h"     /* the reference's host Matrix<BaseFloat> */
#include "cpucompute/vector.h"     /* the reference's host Vector<BaseFloat> (CE's frame mask) */
#include "net/train-opts.h"        /* the reference's NetTrainOptions (src/net/train-opts.h:29-62) */
#include "util/kaldi-io.h"

#include <cstdio>
#include <cstring>
#include <fstream>

#include "eesen_hip.h"
#include "eesen_hip_info.h"

namespace eesen {

inline void HipCheck(int rc) {  /* KALDI_ERR: message + std::runtime_error (src/base/kaldi-error.cc:168-182) */
  if (rc != EESEN_OK) throw std::runtime_error(std::string("eesen_hip: ") + eesen_last_error());
}

/* Which job of how many this process is.  A launcher may say so through RANK / WORLD_SIZE (torch.distributed.run, bench.py);
 * the recipes say it on the trainer's own command line, `--num-jobs=$nj --job-id=JOB` (train_ctc_parallel_h.sh:141-143, JOB
 * substituted by queue.pl), which train-ctc-parallel.cc parses into locals this seam never sees before the first minibatch --
 * so the command line is read here as well (/proc/self/cmdline).  rank = job id - 1. */
struct SeamJob {
  int rank, world;
  SeamJob() : rank(0), world(1) {
    const char* ws = std::getenv("WORLD_SIZE");
    const char* rk = std::getenv("RANK");
    if (ws && rk && std::atoi(ws) > 1) { world = std::atoi(ws); rank = std::atoi(rk); return; }
    std::ifstream f("/proc/self/cmdline", std::ios::binary);
    std::string arg;
    int nj = 1, id = 1;
    while (std::getline(f, arg, '\0')) {
      if (arg.compare(0, 11, "--num-jobs=") == 0) nj = std::atoi(arg.c_str() + 11);
      else if (arg.compare(0, 9, "--job-id=") == 0) id = std::atoi(arg.c_str() + 9);
    }
    if (nj > 1 && id >= 1 && id <= nj) { world = nj; rank = id - 1; }
  }
};
inline const SeamJob& Job() { static const SeamJob j; return j; }

inline int HipDevice() {  /* CuDevice::SelectGpuId (src/gpucompute/cuda-device.cc:73-140): EESEN_DEVICE, else LOCAL_RANK, else job id - 1 */
  const char* e = std::getenv("EESEN_DEVICE");
  if (!e) e = std::getenv("LOCAL_RANK");
  if (e) return std::atoi(e);
  int n = 0;
  if (Job().world > 1 && eesen_device_count(&n) == EESEN_OK && n > 0) return Job().rank % n;
  return 0;
}

/* The one communicator of the process (a job = one rank), created on first need: by Net::SetTrainMode when training, by
 * comm_touch_done when cross-validating (which exchanges nothing but the final counts). */
struct SeamComm {
  eesen_comm_t* comm;
  eesen_net_t* net;   /* the training net the communicator is attached to (NULL: none) */
  SeamComm() : comm(NULL), net(NULL) {}
  ~SeamComm() { if (comm) eesen_comm_destroy(comm); }
  eesen_comm_t* Get() {
    if (!comm && Job().world > 1) {
      const char* addr = std::getenv("MASTER_ADDR");
      const char* cp = std::getenv("EESEN_COMM_PORT");
      const char* mp = std::getenv("MASTER_PORT");
      const int port = cp ? std::atoi(cp) : (mp ? std::atoi(mp) + 17 : 29517);
      HipCheck(eesen_comm_create_tcp(HipDevice(), addr ? addr : "127.0.0.1", port, Job().rank, Job().world, 300, &comm));
    }
    return comm;
  }
};
inline SeamComm& TheComm() { static SeamComm c; return c; }
inline eesen_net_t*& LastNet() { static eesen_net_t* n = NULL; return n; }  /* the process's Net (the trainers hold exactly one) */

/* CuMatrixBase / CuMatrix (src/gpucompute/cuda-matrix.h:39-447): {data, MatrixDim{rows, cols, stride}}.  A CuMatrix built
 * from a host Matrix keeps the HOST pointer (eesen_net_propagate uploads it itself, as the reference's constructor would);
 * otherwise it owns device memory or is a view of memory the Net owns. */
template <typename Real>
class CuMatrixBase {
 public:
  int32 NumRows() const { return rows_; }
  int32 NumCols() const { return cols_; }
  int32 Stride() const { return stride_; }
  const Real* Data() const { return data_; }
  Real* Data() { return data_; }
  bool OnHost() const { return host_; }

 protected:
  CuMatrixBase() : data_(NULL), rows_(0), cols_(0), stride_(0), host_(false) {}
  Real* data_;
  int32 rows_, cols_, stride_;
  bool host_;
};

template <typename Real>
class CuMatrix : public CuMatrixBase<Real> {
 public:
  CuMatrix() : own_(false) {}
  explicit CuMatrix(const MatrixBase<Real>& m) : own_(false) {  /* CuMatrix(const MatrixBase&) cuda-matrix.h:367 */
    this->data_ = const_cast<Real*>(m.Data());
    this->rows_ = m.NumRows(); this->cols_ = m.NumCols(); this->stride_ = m.Stride();
    this->host_ = true;
  }
  ~CuMatrix() { Release(); }
  /* device storage of at least rows x cols, rows 16-byte aligned (callee-resizes-output convention, layer.h:192, ctc-loss.cc:103) */
  void Resize(int32 rows, int32 cols) {
    const int32 ld = (cols + 3) & ~3;
    if (own_ && !this->host_ && (long)rows * ld <= cap_) { this->rows_ = rows; this->cols_ = cols; this->stride_ = ld; return; }
    Release();
    void* p = NULL;
    cap_ = (long)rows * ld;
    HipCheck(eesen_dev_alloc(HipDevice(), cap_ * (long)sizeof(Real), &p));
    this->data_ = static_cast<Real*>(p);
    this->rows_ = rows; this->cols_ = cols; this->stride_ = ld; this->host_ = false;
    own_ = true;
  }
  /* a view of memory owned elsewhere (the Net's output buffer) */
  void View(const Real* p, int32 rows, int32 cols, int32 stride) {
    Release();
    this->data_ = const_cast<Real*>(p);
    this->rows_ = rows; this->cols_ = cols; this->stride_ = stride; this->host_ = false;
  }
  void CopyToMat(Matrix<Real>* dst) const {  /* cuda-matrix.cc CopyToMat */
    dst->Resize(this->rows_, this->cols_);
    for (int32 r = 0; r < this->rows_; ++r)
      HipCheck(eesen_dev_copy(HipDevice(), dst->RowData(r), this->data_ + (size_t)r * this->stride_, (long)this->cols_ * sizeof(Real), 2));
  }

 private:
  CuMatrix(const CuMatrix&);
  CuMatrix& operator=(const CuMatrix&);
  void Release() {
    if (own_ && this->data_) eesen_dev_free(HipDevice(), this->data_);
    this->data_ = NULL; own_ = false; cap_ = 0;
  }
  bool own_;
  long cap_ = 0;
};

/* eesen::Net (src/net/net.h:37-175) for <BiLstmParallel> / <LstmParallel> / <AffineTransform> / <Softmax> stacks */
class Net {
 public:
  Net() : h_(NULL), attached_(false) { HipCheck(eesen_net_create(HipDevice(), NULL, &h_)); LastNet() = h_; }
  ~Net() {
    if (LastNet() == h_) LastNet() = NULL;
    if (attached_) { eesen_net_set_comm(h_, NULL); TheComm().net = NULL; }
    if (h_) eesen_net_destroy(h_);
  }
  void Read(const std::string& file) { HipCheck(eesen_net_read(h_, file.c_str())); }                         /* net.cc:279-309 */
  /* net.cc:325-334.  With several jobs EVERY job of the reference trainer writes the target model (train-ctc-parallel.cc:244-246);
   * behind this seam they hold identical models, so each writes its own temporary file and renames it over the target */
  void Write(const std::string& file, bool binary) const {
    if (Job().world <= 1) { HipCheck(eesen_net_write(h_, file.c_str(), binary)); return; }
    std::ostringstream tmp;
    tmp << file << ".job" << Job().rank + 1 << ".$$";
    HipCheck(eesen_net_write(h_, tmp.str().c_str(), binary));
    if (std::rename(tmp.str().c_str(), file.c_str()) != 0) throw std::runtime_error("eesen_hip: cannot rename " + tmp.str() + " to " + file);
  }
  void SetTrainOptions(const NetTrainOptions& o) {                                                          /* net.h:147-153 */
    HipCheck(eesen_net_set_train_options(h_, o.learn_rate, o.momentum));
    HipCheck(eesen_net_set_adaptive_options(h_, o.adagrad_epsilon, o.rmsprop_rho));
  }
  void SetUpdateAlgorithm(std::string opt) { HipCheck(eesen_net_set_update_algorithm(h_, opt.c_str())); }   /* net.cc:481-497 */
  void SetTrainMode() {                                                                                     /* net.cc:405-412 */
    HipCheck(eesen_net_set_train_mode(h_, 1));
    /* one job of several (SeamJob): join the RCCL communicator; from here on Backpropagate sums the gradients over the jobs
     * (replaces comm_avg_weights, communicator.h:39-119) */
    if (!attached_ && Job().world > 1) {
      HipCheck(eesen_net_set_dropout_seed(h_, 777ull + (unsigned long long)Job().rank));
      HipCheck(eesen_net_set_comm(h_, TheComm().Get()));
      attached_ = true;
      TheComm().net = h_;
    }
  }
  void SetTestMode() { HipCheck(eesen_net_set_train_mode(h_, 0)); }                                         /* net.cc:396-403 */
  void SetSeqLengths(std::vector<int>& lens) { HipCheck(eesen_net_set_seq_lengths(h_, lens.data(), (int)lens.size())); }  /* net.h:157 */
  int32 InputDim() const { int d = 0; HipCheck(eesen_net_input_dim(h_, &d)); return d; }                    /* net.cc:139-142 */
  int32 OutputDim() const { int d = 0; HipCheck(eesen_net_output_dim(h_, &d)); return d; }
  int32 NumParams() const { long n = 0; HipCheck(eesen_net_num_params(h_, &n)); return (int32)n; }
  /* Net::Propagate (net.cc:67-86): `in` is what the trainer builds from the padded host matrix (train-ctc-parallel.cc:198),
   * or a device matrix; *out becomes a view of the Net-owned output, valid until the next Propagate */
  void Propagate(const CuMatrixBase<BaseFloat>& in, CuMatrix<BaseFloat>* out) {
    const float* o = NULL;
    int oc = 0, old = 0;
    HipCheck(eesen_net_propagate(h_, in.Data(), in.NumRows(), in.Stride(), in.OnHost() ? 0 : 1, &o, &oc, &old));
    out->View(o, in.NumRows(), oc, old);
  }
  void Feedforward(const CuMatrixBase<BaseFloat>& in, CuMatrix<BaseFloat>* out) { Propagate(in, out); }     /* net.cc:110-132 */
  /* Net::Backpropagate (net.cc:88-108): gradients, then every layer's Update (:101-104).  With a communicator attached to the
   * handle (eesen_net_set_comm) the per-layer gradient all-reduce runs in between, inside the library. */
  void Backpropagate(const CuMatrixBase<BaseFloat>& out_diff, CuMatrix<BaseFloat>* in_diff) {
    if (in_diff) in_diff->Resize(out_diff.NumRows(), InputDim());
    HipCheck(eesen_net_backpropagate(h_, out_diff.Data(), out_diff.Stride(), in_diff ? in_diff->Data() : NULL, in_diff ? in_diff->Stride() : 0));
    HipCheck(eesen_net_update(h_));
  }
  /* net.cc:336-366: topology, layer markers and the MomentStatistics of every parameter tensor / momentum buffer (device-side
   * reductions, eesen_net_tensor_moments; strings arranged by eesen_hip_info.h) */
  std::string Info() const { return eesen_hip::NetInfo(h_, 0); }
  std::string InfoGradient() const { return eesen_hip::NetInfo(h_, 1); }
  eesen_net_t* Handle() { return h_; }

 private:
  Net(const Net&);
  Net& operator=(const Net&);
  eesen_net_t* h_;
  bool attached_;
};

/* A token n-gram LM for Ctc::DecodeParallel (eesen_lm_*; no counterpart in the reference, whose LM lives in the G of its TLG graphs):
 * an ARPA file whose words are the net's own tokens -- the symbols of units.txt, or decimal class ids when `units` is empty --
 * compiled on the host into a backoff automaton.  num_classes: the net's output dimension, blank included. */
class TokenLm {
 public:
  TokenLm(const std::string& arpa, const std::string& units, int32 num_classes) : h_(NULL) {
    HipCheck(eesen_lm_create_from_arpa(arpa.c_str(), units.empty() ? NULL : units.c_str(), num_classes, &h_));
  }
  ~TokenLm() { if (h_) eesen_lm_destroy(h_); }
  int32 Order() const { int v = 0; HipCheck(eesen_lm_info(h_, &v, NULL, NULL, NULL)); return v; }
  int32 NumStates() const { int v = 0; HipCheck(eesen_lm_info(h_, NULL, &v, NULL, NULL)); return v; }
  int32 NumArcs() const { int v = 0; HipCheck(eesen_lm_info(h_, NULL, NULL, &v, NULL)); return v; }
  bool HasEos() const { int v = 0; HipCheck(eesen_lm_info(h_, NULL, NULL, NULL, &v)); return v != 0; }
  int32 Start() const { int v = 0; HipCheck(eesen_lm_start(h_, &v)); return v; }
  /* lm_step: ln P(c | state) as the fp32 sum the device forms; *next: the state after c */
  BaseFloat Step(int32 state, int32 c, int32* next) const { float w = 0; int n = 0; HipCheck(eesen_lm_step(h_, state, c, &w, &n)); *next = n; return w; }
  BaseFloat Final(int32 state) const { float w = 0; HipCheck(eesen_lm_final(h_, state, &w)); return w; }
  /* ln P(labels [, </s>]) in double on the stored weights */
  double Score(const std::vector<int32>& labels, bool eos = false) const {
    double v = 0;
    HipCheck(eesen_lm_score(h_, labels.empty() ? NULL : labels.data(), (int)labels.size(), eos ? 1 : 0, &v, NULL));
    return v;
  }
  eesen_lm_t* Handle() const { return h_; }

 private:
  TokenLm(const TokenLm&);
  TokenLm& operator=(const TokenLm&);
  eesen_lm_t* h_;
};

/* A lexicon for Ctc::DecodeParallel (eesen_lex_*; no counterpart in the reference, whose lexicon lives in the L of its TLG graphs):
 * `word unit unit ...` lines -- the units are the symbols of units.txt, or decimal class ids when `units` is empty -- compiled on the
 * host into a trie.  num_classes: the net's output dimension, blank included; space_class: the unit that separates words.  Without
 * a space class: the unspaced kind (eesen_lex_create_unspaced) of the phoneme systems -- nothing but CTC's blank between words, several
 * words (homophones) per spelling -- which Ctc::DecodeParallel decodes with eesen_ctc_decode_parallel_words. */
class Lexicon {
 public:
  Lexicon(const std::string& path, const std::string& units, int32 num_classes, int32 space_class) : h_(NULL), space_(space_class) {
    HipCheck(eesen_lex_create(path.c_str(), units.empty() ? NULL : units.c_str(), num_classes, space_class, &h_));
  }
  Lexicon(const std::string& path, const std::string& units, int32 num_classes) : h_(NULL), space_(0) {
    HipCheck(eesen_lex_create_unspaced(path.c_str(), units.empty() ? NULL : units.c_str(), num_classes, &h_));
  }
  bool Unspaced() const { return space_ == 0; }
  int32 SpaceClass() const { return space_; }   /* 0: the unspaced kind */
  int32 MaxHomophones() const { int v = 0; HipCheck(eesen_lex_max_homophones(h_, &v)); return v; }
  /* the ascending ids of the words whose spelling ends at the node */
  std::vector<int32> NodeWords(int32 node) const {
    int n = 0;
    HipCheck(eesen_lex_node_words(h_, node, NULL, 0, &n));
    std::vector<int32> out(n + 1);
    HipCheck(eesen_lex_node_words(h_, node, out.data(), n, &n));
    out.resize(n);
    return out;
  }
  ~Lexicon() { if (h_) eesen_lex_destroy(h_); }
  int32 NumWords() const { int v = 0; HipCheck(eesen_lex_info(h_, &v, NULL, NULL)); return v; }
  int32 NumNodes() const { int v = 0; HipCheck(eesen_lex_info(h_, NULL, &v, NULL)); return v; }
  int32 MaxWordLength() const { int v = 0; HipCheck(eesen_lex_info(h_, NULL, NULL, &v)); return v; }
  /* `word id` lines: the table a word LM is built over, TokenLm(arpa, path, NumWords() + 1) */
  void WriteWords(const std::string& path) const { HipCheck(eesen_lex_write_words(h_, path.c_str())); }
  int32 Child(int32 node, int32 c) const { int v = 0; HipCheck(eesen_lex_child(h_, node, c, &v)); return v; }   /* -1: none */
  int32 Word(int32 node) const { int v = 0; HipCheck(eesen_lex_word(h_, node, &v)); return v; }                /* 0: none ends here */
  /* the word ids of a labelling `w1 space w2 ... wn`; false for a labelling that is none */
  bool Words(const std::vector<int32>& labels, std::vector<int32>* words) const {
    int n = 0;
    words->resize(labels.size() / 2 + 1);
    if (eesen_lex_words(h_, labels.empty() ? NULL : labels.data(), (int)labels.size(), words->data(), &n) != EESEN_OK) { words->clear(); return false; }
    words->resize(n);
    return true;
  }
  /* The unigram look-ahead table of a word LM over this lexicon, eesen_lex_lookahead: one value per trie node, the largest unigram
   * weight among the words whose spelling passes through or ends at the node. */
  std::vector<BaseFloat> Lookahead(const TokenLm& lm) const {
    std::vector<BaseFloat> la(NumNodes());
    HipCheck(eesen_lex_lookahead(h_, lm.Handle(), la.data(), (int)la.size()));
    return la;
  }
  eesen_lex_t* Handle() const { return h_; }

 private:
  Lexicon(const Lexicon&);
  Lexicon& operator=(const Lexicon&);
  eesen_lex_t* h_;
  int32 space_;
};

/* eesen::Ctc (src/net/ctc-loss.h:29-90), the multi-sequence entry points */
class Ctc {
 public:
  Ctc() : h_(NULL), report_step_(100), frames_per_sec_(100.0f), seq_progress_(0), obj_last_(0), err_last_(0), ref_last_(0) {
    HipCheck(eesen_ctc_create(HipDevice(), NULL, &h_));
  }
  ~Ctc() { if (h_) eesen_ctc_destroy(h_); }
  /* ctc-loss.cc:101-194; diff is resized by the callee (:103).  Nothing here waits for the device: ln p joins the objective
   * when it has arrived, as the reference's call only accumulates obj_progress_ (:171-177). */
  void EvalParallel(const std::vector<int32>& frame_num_utt, const CuMatrixBase<BaseFloat>& net_out,
                    std::vector<std::vector<int32> >& label, CuMatrix<BaseFloat>* diff) {
    const int S = (int)frame_num_utt.size();
    Csr(label, S);
    if (!guarded_ && LastNet()) { HipCheck(eesen_ctc_set_guard(h_, LastNet())); guarded_ = true; }  /* a timed-out forward pass never reaches the statistics */
    diff->Resize(net_out.NumRows(), net_out.NumCols());
    HipCheck(eesen_ctc_eval_parallel(h_, frame_num_utt.data(), S, net_out.Data(), net_out.NumRows(), net_out.NumCols(), net_out.Stride(),
                                     ids_.data(), off_.data(), diff->Data(), diff->Stride(), NULL));
    seq_progress_ += S;
    if (seq_progress_ >= report_step_) {  /* :180-192 */
      double obj = 0; long seqs = 0, frames = 0, e = 0, r = 0;
      HipCheck(eesen_ctc_stats(h_, &obj, &seqs, &frames, &e, &r));
      KALDI_VLOG(1) << "After " << seqs << " sequences (" << frames / (frames_per_sec_ * 3600) << "Hr): Obj(log[Pzx]) = "
                    << (obj - obj_last_) / seq_progress_ << "   TokenAcc = " << 100.0 * (1.0 - (double)(e - err_last_) / std::max<long>(r - ref_last_, 1)) << "%";
      obj_last_ = obj; err_last_ = e; ref_last_ = r; seq_progress_ = 0;
    }
  }
  /* ctc-loss.cc:235-298 (returns void: the host part runs deferred, under the device's backward pass) */
  void ErrorRateMSeq(const std::vector<int>& frame_num_utt, const CuMatrixBase<BaseFloat>& net_out, std::vector<std::vector<int> >& label,
                     std::string& out) {
    const int S = (int)frame_num_utt.size();
    Csr(label, S);
    if (out != seq_out_) { HipCheck(eesen_ctc_set_sequence_out_file(h_, out.empty() ? NULL : out.c_str())); seq_out_ = out; }
    HipCheck(eesen_ctc_error_rate_mseq(h_, frame_num_utt.data(), S, net_out.Data(), net_out.NumRows(), net_out.NumCols(), net_out.Stride(),
                                       ids_.data(), off_.data(), NULL, NULL));
  }
  /* Best-path (Viterbi) alignment, eesen_ctc_align_parallel: no counterpart in src/net (the reference aligns through a TLG graph and
   * its decoder, align_ctc_single_utt.sh:67-85).  net_out: posteriors, or log-domain scores with is_log.  ali / pos (pos may be NULL):
   * class id / lattice position of row t*S + s, -1 beyond an utterance's length; score: the path's log-score per utterance, -1e30 (and
   * -1 in every row) where no path exists.  Ties: the smallest move wins, the final blank wins over the last label. */
  void AlignParallel(const std::vector<int32>& frame_num_utt, const CuMatrixBase<BaseFloat>& net_out, std::vector<std::vector<int32> >& label,
                     std::vector<int32>* ali, std::vector<int32>* pos, std::vector<BaseFloat>* score, bool is_log = false) {
    const int S = (int)frame_num_utt.size();
    Csr(label, S);
    if (!guarded_ && LastNet()) { HipCheck(eesen_ctc_set_guard(h_, LastNet())); guarded_ = true; }
    ali->resize(net_out.NumRows());
    if (pos) pos->resize(net_out.NumRows());
    score->resize(S);
    HipCheck(eesen_ctc_align_parallel(h_, frame_num_utt.data(), S, net_out.Data(), net_out.NumRows(), net_out.NumCols(), net_out.Stride(),
                                      is_log ? 1 : 0, ids_.data(), off_.data(), ali->data(), pos ? pos->data() : NULL, score->data()));
  }
  /* Lexicon-free prefix beam search, eesen_ctc_decode_parallel: no counterpart in src/net (the reference decodes through a TLG graph and
   * its WFST decoder).  net_out: posteriors, or log-domain scores with is_log.  hyps[s]: the utterance's labellings, best first (at most
   * nbest; none where the beam died); scores[s]: their log-probabilities. */
  void DecodeParallel(const std::vector<int32>& frame_num_utt, const CuMatrixBase<BaseFloat>& net_out,
                      std::vector<std::vector<std::vector<int32> > >* hyps, std::vector<std::vector<BaseFloat> >* scores, int32 beam = 16,
                      int32 max_classes = 20, int32 nbest = 1, bool is_log = false) {
    const int S = (int)frame_num_utt.size();
    const int T = S > 0 ? net_out.NumRows() / S : 0;
    if (!guarded_ && LastNet()) { HipCheck(eesen_ctc_set_guard(h_, LastNet())); guarded_ = true; }
    last_nbest_ = nbest;
    std::vector<int32> hyp((size_t)S * nbest * T + 1), len((size_t)S * nbest + 1);
    std::vector<BaseFloat> sc((size_t)S * nbest + 1);
    HipCheck(eesen_ctc_decode_parallel(h_, frame_num_utt.data(), S, net_out.Data(), net_out.NumRows(), net_out.NumCols(), net_out.Stride(),
                                       is_log ? 1 : 0, beam, max_classes, nbest, hyp.data(), len.data(), sc.data()));
    hyps->assign(S, std::vector<std::vector<int32> >());
    scores->assign(S, std::vector<BaseFloat>());
    for (int s = 0; s < S; ++s)
      for (int i = 0; i < nbest && len[(size_t)s * nbest + i] >= 0; ++i) {
        const int32* h = hyp.data() + ((size_t)s * nbest + i) * T;
        (*hyps)[s].push_back(std::vector<int32>(h, h + len[(size_t)s * nbest + i]));
        (*scores)[s].push_back(sc[(size_t)s * nbest + i]);
      }
  }
  /* The same search with a token LM fused in, eesen_ctc_decode_parallel_lm: every label adds lm_weight * ln P_lm(label | prefix) +
   * insertion_bonus; with use_eos lm_weight * ln P_lm(</s> | labels) joins at the end.  lm_scores (may be NULL): per returned entry
   * the unweighted ln P_lm of its labels. */
  void DecodeParallel(const std::vector<int32>& frame_num_utt, const CuMatrixBase<BaseFloat>& net_out, const TokenLm& lm, float lm_weight,
                      float insertion_bonus, bool use_eos, std::vector<std::vector<std::vector<int32> > >* hyps,
                      std::vector<std::vector<BaseFloat> >* scores, std::vector<std::vector<BaseFloat> >* lm_scores = NULL, int32 beam = 16,
                      int32 max_classes = 20, int32 nbest = 1, bool is_log = false) {
    const int S = (int)frame_num_utt.size();
    const int T = S > 0 ? net_out.NumRows() / S : 0;
    if (!guarded_ && LastNet()) { HipCheck(eesen_ctc_set_guard(h_, LastNet())); guarded_ = true; }
    last_nbest_ = nbest;
    std::vector<int32> hyp((size_t)S * nbest * T + 1), len((size_t)S * nbest + 1);
    std::vector<BaseFloat> sc((size_t)S * nbest + 1), lsc((size_t)S * nbest + 1);
    HipCheck(eesen_ctc_decode_parallel_lm(h_, frame_num_utt.data(), S, net_out.Data(), net_out.NumRows(), net_out.NumCols(), net_out.Stride(),
                                          is_log ? 1 : 0, beam, max_classes, nbest, lm.Handle(), lm_weight, insertion_bonus, use_eos ? 1 : 0,
                                          hyp.data(), len.data(), sc.data(), lsc.data()));
    hyps->assign(S, std::vector<std::vector<int32> >());
    scores->assign(S, std::vector<BaseFloat>());
    if (lm_scores) lm_scores->assign(S, std::vector<BaseFloat>());
    for (int s = 0; s < S; ++s)
      for (int i = 0; i < nbest && len[(size_t)s * nbest + i] >= 0; ++i) {
        const int32* h = hyp.data() + ((size_t)s * nbest + i) * T;
        (*hyps)[s].push_back(std::vector<int32>(h, h + len[(size_t)s * nbest + i]));
        (*scores)[s].push_back(sc[(size_t)s * nbest + i]);
        if (lm_scores) (*lm_scores)[s].push_back(lsc[(size_t)s * nbest + i]);
      }
  }
  /* The search held to a lexicon, eesen_ctc_decode_parallel_lex: the labellings are lexicon words separated by single spaces.  lm
   * (may be NULL): an LM over the lexicon's word ids (built over Lexicon::WriteWords' table with NumWords() + 1 classes), stepped once
   * per word; every word adds lm_weight * ln P_lm(word | words before) + word_bonus.  words[s][i]: the word ids of hyps[s][i];
   * lm_scores (may be NULL): the unweighted ln P_lm of those words.  An utterance none of whose surviving prefixes ends a word
   * returns nothing. */
  void DecodeParallel(const std::vector<int32>& frame_num_utt, const CuMatrixBase<BaseFloat>& net_out, const Lexicon& lexicon, const TokenLm* lm,
                      float lm_weight, float word_bonus, bool use_eos, std::vector<std::vector<std::vector<int32> > >* hyps,
                      std::vector<std::vector<std::vector<int32> > >* words, std::vector<std::vector<BaseFloat> >* scores,
                      std::vector<std::vector<BaseFloat> >* lm_scores = NULL, int32 beam = 16, int32 max_classes = 20, int32 nbest = 1,
                      bool is_log = false) {
    DecodeParallel(frame_num_utt, net_out, lexicon, lm, lm_weight, word_bonus, use_eos, hyps, words, NULL, scores, lm_scores, beam, max_classes,
                   nbest, is_log);
  }
  /* The same, and word_ends[s][i][j]: the number of labels of hyps[s][i] up to and including word j's last.  An unspaced lexicon takes
   * eesen_ctc_decode_parallel_words: an entry is a labelling and a segmentation of it, both from the device; homophones and other
   * segmentations of the same labels are entries of their own. */
  void DecodeParallel(const std::vector<int32>& frame_num_utt, const CuMatrixBase<BaseFloat>& net_out, const Lexicon& lexicon, const TokenLm* lm,
                      float lm_weight, float word_bonus, bool use_eos, std::vector<std::vector<std::vector<int32> > >* hyps,
                      std::vector<std::vector<std::vector<int32> > >* words, std::vector<std::vector<std::vector<int32> > >* word_ends,
                      std::vector<std::vector<BaseFloat> >* scores, std::vector<std::vector<BaseFloat> >* lm_scores = NULL, int32 beam = 16,
                      int32 max_classes = 20, int32 nbest = 1, bool is_log = false) {
    const int S = (int)frame_num_utt.size();
    const int T = S > 0 ? net_out.NumRows() / S : 0;
    if (!guarded_ && LastNet()) { HipCheck(eesen_ctc_set_guard(h_, LastNet())); guarded_ = true; }
    last_nbest_ = nbest;
    std::vector<int32> hyp((size_t)S * nbest * T + 1), len((size_t)S * nbest + 1), wrd((size_t)S * nbest * T + 1), wlen((size_t)S * nbest + 1);
    std::vector<BaseFloat> sc((size_t)S * nbest + 1), lsc((size_t)S * nbest + 1);
    std::vector<int32> wend(lexicon.Unspaced() ? (size_t)S * nbest * T + 1 : 1);
    if (lexicon.Unspaced())
      HipCheck(eesen_ctc_decode_parallel_words(h_, frame_num_utt.data(), S, net_out.Data(), net_out.NumRows(), net_out.NumCols(), net_out.Stride(),
                                               is_log ? 1 : 0, beam, max_classes, nbest, lexicon.Handle(), lm ? lm->Handle() : NULL, lm_weight,
                                               word_bonus, use_eos ? 1 : 0, hyp.data(), len.data(), sc.data(), lsc.data(), wrd.data(), wlen.data(),
                                               wend.data()));
    else
      HipCheck(eesen_ctc_decode_parallel_lex(h_, frame_num_utt.data(), S, net_out.Data(), net_out.NumRows(), net_out.NumCols(), net_out.Stride(),
                                             is_log ? 1 : 0, beam, max_classes, nbest, lexicon.Handle(), lm ? lm->Handle() : NULL, lm_weight,
                                             word_bonus, use_eos ? 1 : 0, hyp.data(), len.data(), sc.data(), lsc.data(), wrd.data(), wlen.data()));
    hyps->assign(S, std::vector<std::vector<int32> >());
    words->assign(S, std::vector<std::vector<int32> >());
    if (word_ends) word_ends->assign(S, std::vector<std::vector<int32> >());
    scores->assign(S, std::vector<BaseFloat>());
    if (lm_scores) lm_scores->assign(S, std::vector<BaseFloat>());
    for (int s = 0; s < S; ++s)
      for (int i = 0; i < nbest && len[(size_t)s * nbest + i] >= 0; ++i) {
        const size_t e = (size_t)s * nbest + i;
        (*hyps)[s].push_back(std::vector<int32>(hyp.data() + e * T, hyp.data() + e * T + len[e]));
        (*words)[s].push_back(std::vector<int32>(wrd.data() + e * T, wrd.data() + e * T + wlen[e]));
        if (word_ends && lexicon.Unspaced()) (*word_ends)[s].push_back(std::vector<int32>(wend.data() + e * T, wend.data() + e * T + wlen[e]));
        if (word_ends && !lexicon.Unspaced()) {   /* a word ends in front of every space and at the end */
          std::vector<int32> ends;
          for (int j = 0; j < len[e]; ++j)
            if (hyp[e * T + j] == lexicon.SpaceClass()) ends.push_back(j);
          if (len[e] > 0) ends.push_back(len[e]);
          (*word_ends)[s].push_back(ends);
        }
        (*scores)[s].push_back(sc[e]);
        if (lm_scores) (*lm_scores)[s].push_back(lsc[e]);
      }
  }
  /* eesen_ctc_set_lm_lookahead: 0 = off, 1 = the DecodeParallel overloads that take a Lexicon and a TokenLm rank a frame's candidates
   * with the unigram look-ahead (INTEGRATION.md "LM look-ahead"); it stays set.  With 1 a lexicon call without an LM is refused. */
  void SetLmLookahead(int32 mode) { HipCheck(eesen_ctc_set_lm_lookahead(h_, mode)); }
  int32 LmLookahead() const { int v = 0; HipCheck(eesen_ctc_get_lm_lookahead(h_, &v)); return v; }
  /* Time stamps and confidences of the entries the LAST DecodeParallel returned (any overload), eesen_ctc_decode_stamps: every entry is
   * aligned on the acoustic scores by AlignParallel's recurrence and tie rule, all of them in one launch.  frame_num_utt, net_out,
   * is_log: that call's; hyps: what it returned.  Per utterance s and returned entry i: label_start / label_end [labels] the frames
   * [start, end) of every label; word_start / word_end / word_conf [words] the frames of every word (a label, a run between spaces, or
   * a run up to a word end, by the call's kind) and its N-best posterior with conf_scale on the totals; path_score the best path's
   * log-score (0 for the empty labelling). */
  struct Stamps {
    std::vector<std::vector<std::vector<int32> > > label_start, label_end, word_start, word_end;
    std::vector<std::vector<std::vector<BaseFloat> > > word_conf;
    std::vector<std::vector<BaseFloat> > path_score;
  };
  void DecodeStamps(const std::vector<int32>& frame_num_utt, const CuMatrixBase<BaseFloat>& net_out,
                    const std::vector<std::vector<std::vector<int32> > >& hyps, Stamps* out, bool is_log = false, double conf_scale = 1.0) {
    const int S = (int)frame_num_utt.size(), nbest = last_nbest_;
    const int T = S > 0 ? net_out.NumRows() / S : 0;
    const size_t n = (size_t)S * nbest * T + 1;
    std::vector<int32> ls(n), le(n), ws(n), we(n);
    std::vector<BaseFloat> wc(n), ps((size_t)S * nbest + 1);
    HipCheck(eesen_ctc_decode_stamps(h_, frame_num_utt.data(), S, net_out.Data(), net_out.NumRows(), net_out.NumCols(), net_out.Stride(),
                                     is_log ? 1 : 0, conf_scale, ls.data(), le.data(), ws.data(), we.data(), wc.data(), ps.data()));
    out->label_start.assign(S, std::vector<std::vector<int32> >());
    out->label_end = out->word_start = out->word_end = out->label_start;
    out->word_conf.assign(S, std::vector<std::vector<BaseFloat> >());
    out->path_score.assign(S, std::vector<BaseFloat>());
    for (int s = 0; s < S && s < (int)hyps.size(); ++s)
      for (int i = 0; i < nbest && i < (int)hyps[s].size(); ++i) {
        const size_t e = ((size_t)s * nbest + i) * T;
        const size_t nl = hyps[s][i].size() < (size_t)T ? hyps[s][i].size() : (size_t)T;
        size_t nw = 0;
        while (nw < (size_t)T && wc[e + nw] != -1e30f) ++nw;   /* -1e30 beyond the entry's words */
        out->label_start[s].push_back(std::vector<int32>(ls.data() + e, ls.data() + e + nl));
        out->label_end[s].push_back(std::vector<int32>(le.data() + e, le.data() + e + nl));
        out->word_start[s].push_back(std::vector<int32>(ws.data() + e, ws.data() + e + nw));
        out->word_end[s].push_back(std::vector<int32>(we.data() + e, we.data() + e + nw));
        out->word_conf[s].push_back(std::vector<BaseFloat>(wc.data() + e, wc.data() + e + nw));
        out->path_score[s].push_back(ps[(size_t)s * nbest + i]);
      }
  }
  /* Exact log-scores ln p(labels | x), eesen_ctc_score_parallel (INTEGRATION.md "Rescoring"): hyps[s] any labellings of utterance s
   * (an empty one: the empty labelling); scores[s][i] that of hyps[s][i], -1e30 (read <= -1e29) where it has no path. */
  void ScoreParallel(const std::vector<int32>& frame_num_utt, const CuMatrixBase<BaseFloat>& net_out,
                     const std::vector<std::vector<std::vector<int32> > >& hyps, std::vector<std::vector<BaseFloat> >* scores,
                     bool is_log = false) {
    const int S = (int)frame_num_utt.size();
    std::vector<int> hoff(1, 0), loff(1, 0), ids;
    for (int s = 0; s < S && s < (int)hyps.size(); ++s) {
      for (size_t i = 0; i < hyps[s].size(); ++i) {
        ids.insert(ids.end(), hyps[s][i].begin(), hyps[s][i].end());
        loff.push_back((int)ids.size());
      }
      hoff.push_back((int)loff.size() - 1);
    }
    while ((int)hoff.size() < S + 1) hoff.push_back(hoff.back());
    if (ids.empty()) ids.push_back(0);
    std::vector<BaseFloat> sc(loff.size());
    HipCheck(eesen_ctc_score_parallel(h_, frame_num_utt.data(), S, net_out.Data(), net_out.NumRows(), net_out.NumCols(), net_out.Stride(),
                                      is_log ? 1 : 0, hoff.data(), loff.data(), ids.data(), sc.data()));
    scores->assign(S, std::vector<BaseFloat>());
    for (int s = 0; s < S; ++s) (*scores)[s].assign(sc.begin() + hoff[s], sc.begin() + hoff[s + 1]);
  }
  /* Second pass over the entries the LAST DecodeParallel returned (any overload), eesen_ctc_decode_rescore: am_score the exact
   * ln p(labels | x), lm_score the fp64 score of `lm` (may be NULL: the first pass's LM sums) over the entry's labels or, after a
   * lexicon call, words, total = am + lm_weight * lm + bonus * tokens; order[s] the first-pass ranks by total, best first, ties to
   * the smaller rank, entries without a path last.  frame_num_utt, net_out, is_log: that call's; hyps: what it returned (every array
   * is cut to the utterance's count). */
  struct Rescored {
    std::vector<std::vector<BaseFloat> > am_score, lm_score, total;
    std::vector<std::vector<int32> > order;
  };
  void RescoreNbest(const std::vector<int32>& frame_num_utt, const CuMatrixBase<BaseFloat>& net_out,
                    const std::vector<std::vector<std::vector<int32> > >& hyps, Rescored* out, const TokenLm* lm = NULL, float lm_weight = 1.0f,
                    float bonus = 0.0f, bool use_eos = false, bool is_log = false) {
    const int S = (int)frame_num_utt.size(), nbest = last_nbest_;
    const size_t n = (size_t)S * nbest + 1;
    std::vector<BaseFloat> am(n), ls(n), tot(n);
    std::vector<int32> ord(n);
    HipCheck(eesen_ctc_decode_rescore(h_, frame_num_utt.data(), S, net_out.Data(), net_out.NumRows(), net_out.NumCols(), net_out.Stride(),
                                      is_log ? 1 : 0, lm ? lm->Handle() : NULL, lm_weight, bonus, use_eos ? 1 : 0, am.data(), ls.data(), tot.data(),
                                      ord.data()));
    out->am_score.assign(S, std::vector<BaseFloat>());
    out->lm_score = out->total = out->am_score;
    out->order.assign(S, std::vector<int32>());
    for (int s = 0; s < S && s < (int)hyps.size(); ++s) {
      const int count = (int)hyps[s].size() < nbest ? (int)hyps[s].size() : nbest;
      for (int i = 0; i < count; ++i) {
        const size_t e = (size_t)s * nbest + i;
        out->am_score[s].push_back(am[e]);
        out->lm_score[s].push_back(ls[e]);
        out->total[s].push_back(tot[e]);
      }
      for (int i = 0; i < nbest; ++i)   /* the ranks beyond the count come last in the library's order: dropped */
        if (ord[(size_t)s * nbest + i] >= 0 && ord[(size_t)s * nbest + i] < count) out->order[s].push_back(ord[(size_t)s * nbest + i]);
    }
  }
  /* Levenshtein distances on the device, eesen_edit_distance_parallel (INTEGRATION.md "Minimum Bayes risk"): seqs[g] the sequences of
   * group g (any int32 tokens, at most 8192 each); pair[g] the n_g x n_g distances among them, row-major; with refs (one per group)
   * ref_dist[g][i] the distance of seqs[g][i] to refs[g].  pair may be NULL (no pairwise distances are computed); refs and ref_dist
   * go together: with either NULL no reference distances are computed. */
  void EditDistanceParallel(const std::vector<std::vector<std::vector<int32> > >& seqs, std::vector<std::vector<int32> >* pair,
                            const std::vector<std::vector<int32> >* refs = NULL, std::vector<std::vector<int32> >* ref_dist = NULL) {
    const int G = (int)seqs.size();
    std::vector<int> soff(1, 0), toff(1, 0), ids, roff(1, 0), rids;
    size_t n2 = 0;
    for (int g = 0; g < G; ++g) {
      for (size_t i = 0; i < seqs[g].size(); ++i) {
        ids.insert(ids.end(), seqs[g][i].begin(), seqs[g][i].end());
        toff.push_back((int)ids.size());
      }
      soff.push_back((int)toff.size() - 1);
      n2 += seqs[g].size() * seqs[g].size();
      if (refs && g < (int)refs->size()) rids.insert(rids.end(), (*refs)[g].begin(), (*refs)[g].end());
      roff.push_back((int)rids.size());
    }
    ids.push_back(0); rids.push_back(0);
    const bool with_refs = refs != NULL && ref_dist != NULL;
    std::vector<int32> p(pair ? n2 + 1 : 1), rd(toff.size());
    HipCheck(eesen_edit_distance_parallel(h_, G, soff.data(), toff.data(), ids.data(), with_refs ? roff.data() : NULL, with_refs ? rids.data() : NULL,
                                          pair ? p.data() : NULL, with_refs ? rd.data() : NULL));
    if (pair) pair->assign(G, std::vector<int32>());
    if (ref_dist) ref_dist->assign(G, std::vector<int32>());
    size_t at = 0;
    for (int g = 0; g < G; ++g) {
      const size_t n = seqs[g].size();
      if (pair) (*pair)[g].assign(p.begin() + at, p.begin() + at + n * n);
      at += n * n;
      if (with_refs) (*ref_dist)[g].assign(rd.begin() + soff[g], rd.begin() + soff[g + 1]);
    }
  }
  /* Minimum Bayes risk over the entries the LAST DecodeParallel returned (any overload), eesen_ctc_decode_mbr: dist[s] the nbest x nbest
   * distances (row-major, -1 where an entry does not count), posterior / risk [s][i] (-1e30 there), order[s] the first-pass ranks by
   * risk ascending (ties: the larger score, then the smaller rank; the entries that do not count last), ref_dist[s][i] the distance to
   * refs[s] (empty without refs).  level 0: over the mode's LM tokens, 1: over labels.  totals: z of every entry, S rows of nbest
   * (RescoreNbest's totals padded with -1e30), or NULL for the decode call's scores.  S: that call's. */
  struct Mbr {
    std::vector<std::vector<int32> > dist, ref_dist, order;
    std::vector<std::vector<double> > posterior, risk;
  };
  void MbrNbest(int32 S, Mbr* out, int level = 0, double scale = 1.0, const std::vector<std::vector<BaseFloat> >* totals = NULL,
                const std::vector<std::vector<int32> >* refs = NULL) {
    const int nbest = last_nbest_;
    const size_t n = (size_t)S * nbest;
    std::vector<BaseFloat> z(n + 1, -1e30f);
    if (totals)
      for (int s = 0; s < S && s < (int)totals->size(); ++s)
        for (int i = 0; i < nbest && i < (int)(*totals)[s].size(); ++i) z[(size_t)s * nbest + i] = (*totals)[s][i];
    std::vector<int> roff(1, 0), rids;
    for (int s = 0; s < S; ++s) {
      if (refs && s < (int)refs->size()) rids.insert(rids.end(), (*refs)[s].begin(), (*refs)[s].end());
      roff.push_back((int)rids.size());
    }
    rids.push_back(0);
    std::vector<int32> d(n * nbest + 1), rd(n + 1), ord(n + 1);
    std::vector<double> post(n + 1), risk(n + 1);
    HipCheck(eesen_ctc_decode_mbr(h_, S, level, scale, totals ? z.data() : NULL, refs ? roff.data() : NULL, refs ? rids.data() : NULL, d.data(),
                                  refs ? rd.data() : NULL, post.data(), risk.data(), ord.data()));
    out->dist.assign(S, std::vector<int32>());
    out->ref_dist = out->order = out->dist;
    out->posterior.assign(S, std::vector<double>());
    out->risk = out->posterior;
    for (int s = 0; s < S; ++s) {
      const size_t e = (size_t)s * nbest;
      out->dist[s].assign(d.begin() + e * nbest, d.begin() + (e + nbest) * nbest);
      out->order[s].assign(ord.begin() + e, ord.begin() + e + nbest);
      out->posterior[s].assign(post.begin() + e, post.begin() + e + nbest);
      out->risk[s].assign(risk.begin() + e, risk.begin() + e + nbest);
      if (refs) out->ref_dist[s].assign(rd.begin() + e, rd.begin() + e + nbest);
    }
  }
  void SetReportStep(int32 s) { report_step_ = s; }
  void SetFramesPerSec(float f) { frames_per_sec_ = f; }
  float NumErrorTokens() const { long e = 0; HipCheck(eesen_ctc_stats(h_, NULL, NULL, NULL, &e, NULL)); return (float)e; }   /* ctc-loss.h:62 */
  int32 NumRefTokens() const { long r = 0; HipCheck(eesen_ctc_stats(h_, NULL, NULL, NULL, NULL, &r)); return (int32)r; }
  std::string Report() {  /* ctc-loss.cc:300-304; the line train_ctc_parallel.sh:146,158 greps */
    std::ostringstream oss;
    oss << "\nTOKEN_ACCURACY >> " << 100.0 * (1.0 - NumErrorTokens() / NumRefTokens()) << "% <<";
    return oss.str();
  }

 private:
  void Csr(const std::vector<std::vector<int32> >& label, int S) {  /* vector<vector<int32>> -> CSR */
    ids_.clear(); off_.assign(1, 0);
    for (int s = 0; s < S; ++s) { ids_.insert(ids_.end(), label[s].begin(), label[s].end()); off_.push_back((int)ids_.size()); }
    if (ids_.empty()) ids_.push_back(0);
  }
  eesen_ctc_t* h_;
  int32 report_step_;
  float frames_per_sec_;
  long seq_progress_;
  double obj_last_;
  long err_last_, ref_last_;
  std::vector<int> ids_, off_;
  std::string seq_out_;
  bool guarded_ = false;
  int32 last_nbest_ = 1;   /* of the last DecodeParallel: the row count of DecodeStamps' arrays */
};

/* eesen::CE (src/net/ce-loss.h:32-77): frame-level cross-entropy, one fused pass on the device (eesen_ce_eval_parallel) fed by
 * int32 targets instead of the reference's dense one-hot matrix.  Nothing here waits for the device: the progress lines of
 * ce-loss.cc:153-167 are printed (KALDI_LOG, the reference's text) as soon as the sums of the call that produced them have arrived. */
class CE {
 public:
  CE() : h_(NULL), guarded_(false) { HipCheck(eesen_ce_create(HipDevice(), NULL, &h_)); }
  ~CE() { if (h_) eesen_ce_destroy(h_); }
  /* ce-loss.cc:30-92: one sequence, every row valid */
  void Eval(const CuMatrixBase<BaseFloat>& net_out, const std::vector<int32>& target, CuMatrix<BaseFloat>* diff) {
    lens_.assign(1, net_out.NumRows());
    Run(net_out, target, diff, 1);
  }
  /* ce-loss.cc:94-169.  The library takes sequence lengths (row t*S + s valid iff t < len[s]); the seam has the trainer's 0/1
   * frame_mask_host (train-ce-parallel.cc:143-151), which is converted: len[s] = the valid rows of column s, and a mask that is
   * not of that shape -- a 1 after a 0 within a sequence -- is refused (KALDI_ERR semantics). */
  void EvalParallel(const CuMatrixBase<BaseFloat>& net_out, const std::vector<int32>& target, CuMatrix<BaseFloat>* diff,
                    const VectorBase<BaseFloat>& frame_mask_host, int sequence_number_in_batch) {
    const int S = sequence_number_in_batch, rows = net_out.NumRows();
    if (S <= 0 || rows % S != 0 || frame_mask_host.Dim() != rows)
      throw std::runtime_error("eesen_hip: CE::EvalParallel: the frame mask must have one entry per row of S interleaved sequences");
    lens_.assign(S, 0);
    for (int s = 0; s < S; ++s) {
      int t = 0;
      while (t < rows / S && frame_mask_host(t * S + s) == 1.0) ++t;
      lens_[s] = t;
      for (; t < rows / S; ++t)
        if (frame_mask_host(t * S + s) != 0.0)
          throw std::runtime_error("eesen_hip: CE::EvalParallel: the frame mask of a sequence must be 1 on its first frames and 0 after them");
    }
    Run(net_out, target, diff, S);
  }
  void SetReportStep(int32 report_step) { HipCheck(eesen_ce_set_report_step(h_, report_step)); }   /* ce-loss.h:47 */
  /* ce-loss.cc:171-175, with the true ratio correct / frames (the reference's int32 division prints 0 or 100) */
  std::string Report() {
    Progress(1);
    char buf[256];
    HipCheck(eesen_ce_report(h_, buf, (int)sizeof(buf)));
    return buf;
  }

 private:
  CE(const CE&);
  CE& operator=(const CE&);
  void Run(const CuMatrixBase<BaseFloat>& net_out, const std::vector<int32>& target, CuMatrix<BaseFloat>* diff, int S) {
    if ((int)target.size() != net_out.NumRows()) throw std::runtime_error("eesen_hip: CE: one target per row of the network output");
    if (!guarded_ && LastNet()) { HipCheck(eesen_ce_set_guard(h_, LastNet())); guarded_ = true; }  /* a timed-out forward pass never reaches the statistics */
    diff->Resize(net_out.NumRows(), net_out.NumCols());
    HipCheck(eesen_ce_eval_parallel(h_, lens_.data(), S, net_out.Data(), net_out.NumRows(), net_out.NumCols(), net_out.Stride(),
                                    target.data(), diff->Data(), diff->Stride(), NULL));
    Progress(0);
  }
  void Progress(int wait) {
    char buf[4096];
    for (;;) {
      HipCheck(eesen_ce_progress(h_, wait, buf, (int)sizeof(buf)));
      if (!buf[0]) break;
      KALDI_LOG << buf;
    }
  }
  eesen_ce_t* h_;
  bool guarded_;
  std::vector<int> lens_;
};

/* src/net/communicator.h: the multi-job mode of the reference trainer (--num-jobs / --job-id / --utts-per-avg) averages MODELS
 * through files.  Behind this seam a job is one rank of an RCCL communicator that sums GRADIENTS every minibatch inside
 * eesen_net_backpropagate (eesen_net_set_comm): the jobs hold identical models at every step, so "averaging" is the identity.
 * What is left of the protocol happens where the reference trainer calls comm_touch_done, once, after its loop
 * (train-ctc-parallel.cc:226-232):
 *   * jobs with FEWER minibatches than others (the recipes' per-job lists are only approximately even, prep_scps.sh:37-76;
 *     the reference lets a sub-job "give up if the main job finishes first", communicator.h:104-112) keep stepping here with a
 *     zero gradient through the same collectives until no job had a minibatch in a step (eesen_net_live_ranks); the closing
 *     round leaves the model untouched, so the result equals one process on the union of the minibatches;
 *   * the jobs' error / reference token counts are summed over the communicator (the done-files of communicator.h:121-170)
 *     and job 1 prints the `TOTAL TOKEN_ACCURACY` line the recipes grep in its log (train_ctc_parallel_h.sh:147,171). */
inline std::string comm_done_filename(const std::string& base, int job_id) {  /* communicator.h:29-31 */
  std::ostringstream os;
  os << base << ".done.job" << job_id;
  return os.str();
}
inline std::string comm_avg_model_name(const std::string& base, int count) {  /* communicator.h:33-35 */
  std::ostringstream os;
  os << base << ".avg" << count;
  return os.str();
}
inline void comm_avg_weights(Net&, const int&, const int&, const int&, const std::string&, const std::string&) {}  /* communicator.h:39-119 */
inline void comm_touch_done(Ctc& ctc, const int& job_id, const int& num_jobs, const std::string& base_done_filename) {  /* communicator.h:121-170 */
  KALDI_LOG << "Writing done file for job" << job_id;
  {  /* :125-129: the file itself, for whoever looks at the experiment directory */
    std::ofstream out(comm_done_filename(base_done_filename, job_id).c_str());
    out << "Errors " << ctc.NumErrorTokens() << " Refs " << ctc.NumRefTokens();
  }
  if (num_jobs <= 1 || Job().world <= 1) return;
  eesen_comm_t* comm = TheComm().Get();
  if (TheComm().net) {  /* a training job: out of minibatches, others may not be */
    long zero_steps = 0;
    for (;;) {
      int live = 0;
      HipCheck(eesen_net_backpropagate_zero(TheComm().net));
      HipCheck(eesen_net_update(TheComm().net));
      HipCheck(eesen_net_live_ranks(TheComm().net, &live));
      if (live == 0) break;
      ++zero_steps;
    }
    if (zero_steps) KALDI_LOG << "job " << job_id << " ran out of minibatches " << zero_steps << " step(s) before the last job";
  }
  double tot[2] = {(double)ctc.NumErrorTokens(), (double)ctc.NumRefTokens()};
  HipCheck(eesen_comm_allreduce_host(comm, tot, 2, 0));
  if (job_id == 1) {  /* :132, :168 */
    KALDI_LOG << "Collecting stats from " << num_jobs << " done files";
    KALDI_LOG << "\nTOTAL TOKEN_ACCURACY >> " << 100.0 * (1.0 - tot[0] / tot[1]) << "% <<";
  }
}

}  // namespace eesen
#endif  /* EESEN_HIP_NET_H_ */
