// ctc_decode.hip -- CTC prefix beam search over a padded utterance batch, lexicon-free or along a lexicon trie, for gfx950.
//
// No counterpart in the reference, which decodes one utterance per process through a TLG graph and its WFST decoder.  The
// computation is stated in INTEGRATION.md "Decoding" and "LM fusion" and restated in numpy in tests/ctc_beam_restatement.py and
// tests/ctc_lm_restatement.py; the lexicon mode in INTEGRATION.md "Lexicon" and tests/ctc_lex_restatement.py.  Three launches per
// minibatch, whatever the mode, none per frame:
//   ctc_row_topc_kernel     one wavefront per row: the C' best non-blank classes (ascending id), their scores, the blank's score
//   ctc_prefix_beam_kernel  one workgroup per utterance walks its n frames: beam state and the frame's candidate keys in LDS, the trie
//                           of surviving prefixes written (never read) to global memory; <false> the plain search, <true> the
//                           LM-fused one, ctc_prefix_beam_lex_kernel the one that extends only along a lexicon trie and steps a
//                           word LM once per word: one text (prefix_beam<mode>), and a mode's arguments, LDS and barrier exist in
//                           that instantiation only
//   ctc_hyp_kernel          one lane per (utterance, rank) walks the trie to the root
// Along a lexicon without a boundary unit (INTEGRATION.md "Words without a boundary unit", tests/ctc_words_restatement.py) the second
// and third launch are ctc_word_beam_kernel (its text: ctc_word_beam.inc) and ctc_word_hyp_kernel, at the end of this file: hypotheses
// are labels and the words closed between them, and labels, words and word ends all come out of the trie on the device.
// With the unigram LM look-ahead (INTEGRATION.md "LM look-ahead", tests/ctc_lookahead_restatement.py) the two lexicon searches run
// ctc_prefix_beam_lex_la_kernel / ctc_word_beam_la_kernel: the same two texts behind a compile-time flag, the keys alone differ.
// Every log-mass is an fp32 value in [-1e30, +inf): sums are clamped from below at the library's finite sentinel, so the sweep's
// branch-free log-add (ctc.hip: LogAPlusB_fast) is exact on the special cases here too.
#include "kernels.h"
#include "lex.h"
#include "lm.h"

namespace eesen {
namespace {

constexpr float kLogZero = -1e30f, kDead = -1e29f;
constexpr int kMaxBeam = 64, kMaxCls = 64, kMaxKeys = 4096;
constexpr unsigned long long kDeadKey = ~0ull;

// A prefix is known by a 64-bit fingerprint of its labels and its length: h(p + c) = h(p) * M + (c + 1) mod 2^64, M odd, so the
// parent's fingerprint is (h - (c + 1)) * M^-1 -- the merge test needs neither the sequences nor the trie.
constexpr unsigned long long kHashMul = 0x9E3779B97F4A7C15ull;
constexpr unsigned long long inv_mod_2_64(unsigned long long a) {
  unsigned long long x = a;   // Newton: 3 correct bits double five times over
  for (int i = 0; i < 6; ++i) x *= 2 - a * x;
  return x;
}
constexpr unsigned long long kHashMulInv = inv_mod_2_64(kHashMul);
static_assert(kHashMul * kHashMulInv == 1ull, "inverse of the fingerprint multiplier");

__device__ __forceinline__ float clamp_score(float v) { return fmaxf(v, kLogZero); }   // (a NaN becomes the sentinel too)
__device__ __forceinline__ float log_add(float a, float b) {
  const float m = fmaxf(a, b), n = fminf(a, b);
  return m + __logf(1.f + __expf(n - m));
}
__device__ __forceinline__ float score_add(float a, float b) { return fmaxf(a + b, kLogZero); }
// the look-ahead's rank term of a candidate on a lexicon node whose table value is l (INTEGRATION.md "LM look-ahead")
__device__ __forceinline__ float eta_of(float alpha, float beta, float l) { return __fadd_rn(__fmul_rn(alpha, l), beta); }
// order-preserving map of a float onto an unsigned: a < b  <=>  ord(a) < ord(b)
__device__ __forceinline__ unsigned ord(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// selection key: smaller is better -- the total descending, then the tie-rule index ascending
__device__ __forceinline__ unsigned long long make_key(float total, unsigned idx) {
  return ((unsigned long long)(~ord(total)) << 32) | idx;
}

// ---- candidate classes of every frame ------------------------------------------------------------------------------------------
// The C'-th largest key among classes 1 .. K-1 by bisection on the 32 key bits (a count per bit), then one pass in class order that
// keeps what lies above it and the first `need` classes that equal it: ties go to the smaller id and the output is in ascending id
// order by construction.  REG: K <= 256, the row's keys stay in four registers per lane; otherwise the row is re-read per pass (it
// stays in L1/L2: at most 80 KB).
template <bool REG>
__global__ __launch_bounds__(256) void ctc_row_topc_kernel(const float* __restrict__ sc, int ld, int rows, int K, int S,
                                                           const int* __restrict__ lens, int Cc, int* __restrict__ cid,
                                                           float* __restrict__ csc, float* __restrict__ sblank) {
  constexpr int VPL = 4;
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  if (r / S >= lens[r % S]) return;   // a frame beyond its utterance: never read
  const float* row = sc + (size_t)r * ld;
  // key of class k; 0 (below every clamped value's key) for the blank and beyond the row
  auto key_of = [&](int k) -> unsigned { return (k >= 1 && k < K) ? ord(clamp_score(row[k])) : 0u; };
  unsigned u[VPL];
  if constexpr (REG) {
#pragma unroll
    for (int i = 0; i < VPL; ++i) u[i] = key_of(lane + 64 * i);
  }
  auto count = [&](auto pred) -> int {   // classes whose key satisfies pred (wave-uniform)
    int c = 0;
    if constexpr (REG) {
#pragma unroll
      for (int i = 0; i < VPL; ++i) c += __popcll(__ballot(pred(u[i])));
    } else {
      for (int base = 0; base < K; base += 64) c += __popcll(__ballot(pred(key_of(base + lane))));
    }
    return c;
  };
  unsigned tau = 0;
  for (int bit = 31; bit >= 0; --bit) {
    const unsigned cand = tau | (1u << bit);
    if (count([&](unsigned k) { return k >= cand; }) >= Cc) tau = cand;
  }
  const int need = Cc - count([&](unsigned k) { return k > tau; });   // >= 1 of the classes that equal the threshold
  const unsigned long long below = (1ull << lane) - 1;
  int n_out = 0, n_eq = 0;
  int* ids = cid + (size_t)r * Cc;
  float* vals = csc + (size_t)r * Cc;
  auto emit = [&](int k, unsigned key) {
    const bool eq = key == tau;
    const unsigned long long eqm = __ballot(eq);
    const bool take = key > tau || (eq && n_eq + __popcll(eqm & below) < need);
    const unsigned long long tm = __ballot(take);
    const int at = n_out + __popcll(tm & below);
    if (take && at < Cc) { ids[at] = k; vals[at] = clamp_score(row[k]); }
    n_eq += __popcll(eqm);
    n_out += __popcll(tm);
  };
  if constexpr (REG) {
#pragma unroll
    for (int i = 0; i < VPL; ++i) emit(lane + 64 * i, u[i]);
  } else {
    for (int base = 0; base < K; base += 64) emit(base + lane, key_of(base + lane));
  }
  if (lane == 0) sblank[r] = clamp_score(row[0]);
}

// ---- the beam ------------------------------------------------------------------------------------------------------------------
struct BeamState {
  float lb[kMaxBeam], lnb[kMaxBeam];   // log-mass ending in blank / in the last label
  float se[kMaxBeam];                  // this frame's score of the entry's own last label
  int node[kMaxBeam], last[kMaxBeam], len[kMaxBeam];   // trie node, last label (-1: the empty prefix), length
  unsigned long long hash[kMaxBeam];   // fingerprint of the labels
};

// The kernel's modes, and what each has that the plain one has not, as arguments (flm [S][B]: the LM sum of each final entry).  The
// lexicon mode's LM is over word ids (class w = word w) and optional: have_lm == 0 never touches tab.
enum BeamMode { kPlain = 0, kTokenLm = 1, kLexicon = 2 };
template <int MODE> struct LmArgs {};
template <> struct LmArgs<kTokenLm> { LmTables tab; float alpha, beta; int use_eos; float* flm; };
template <> struct LmArgs<kLexicon> { LmTables tab; float alpha, beta; int use_eos; float* flm; LexTables lex; int have_lm; };
// first index in [lo, hi) of the ascending v whose value is >= x; hi if there is none
__device__ __forceinline__ int lower_bound(const int* __restrict__ v, int lo, int hi, int x) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (v[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// lm_step of lm.h on the device copy of the tables (read-only global memory), as TokenLm::step does it on the host.  A level is the
// state's record (one 16-byte load), a bisection of its sorted arc list, and on a hit the arc's (w, next) pair (one 8-byte load);
// state 0 is an index.  Every lane walks a state and a class of its own, so each load is up to 64 scattered requests, and the pass
// is paid by their number (profiles/ctc_decode_lm.md).  The backoff chain of a compiled model ends in state 0; the level bound only
// keeps a walk over tables that are not a model's from running on.
__device__ __forceinline__ void lm_step(const LmTables& L, int state, int c, float& w, int& next) {
  const int4* __restrict__ rec = reinterpret_cast<const int4*>(L.state_rec);
  const int2* __restrict__ wn = reinterpret_cast<const int2*>(L.arc_wn);
  const int* __restrict__ cls = L.arc_cls;
  float acc = 0.f;
  int at = c - 1;   // state 0's arc of class c
  for (int level = 0; level < 8 && state != 0; ++level) {
    const int4 r = rec[state];
    const int end = r.x + r.y;
    const int lo = lower_bound(cls, r.x, end, c);
    if (lo < end && cls[lo] == c) { at = lo; break; }
    acc = __fadd_rn(acc, __int_as_float(r.w));
    state = r.z;
  }
  const int2 a = wn[at];
  w = __fadd_rn(acc, __int_as_float(a.x));
  next = a.y;
}

// Between two sort stages whose strides are both <= 64 a wave re-reads only what it wrote itself (pair q of a stage touches the
// 128-element block q / 64, and a wave keeps its pairs from stage to stage): LDS operations of one wave execute in order, so
// only the compiler's schedule has to be pinned.
__device__ __forceinline__ void sort_sync(bool wave_local) {
  if (wave_local) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  } else {
    __syncthreads();
  }
}

// Grid (S), 64 .. 512 threads.  Frame t of an utterance, between workgroup barriers:
//   0  LM only: one thread per (entry, candidate), nb * C' <= 2048 of them: (w, next) = lm_step(entry's LM state, class) into LDS --
//      the only LM lookups of the frame; steps 1, 2 and 4 read w from there and form g = alpha * w + beta.  Lexicon: the same
//      slots take (0, child of the entry's lexicon node) for a unit and (lm_step over the word LM, or 0, of the node's word) for
//      the space; next = -1 marks a pair the lexicon does not allow, which ext_value turns into -1e30: no candidate
//   1  entry q < nb: its stay candidate; the extension that spells q (found by fingerprint) is log-added into it and marked merged
//   2  the nb * C' extensions write their keys behind the stays; the key array is padded with dead keys to a power of two
//   3  bitonic sort of the keys (workgroup barriers only around strides >= 128)
//   4  rank r < B takes key r: a stay copies its entry, an extension becomes trie node 1 + t * B + r
// The next frame's candidates and the scores of the labels an entry can end in next (its own last label or one of this frame's
// candidates) are fetched at the top of the frame and land in LDS just before step 4, off the dependent chain.
// LM: shallow fusion (INTEGRATION.md "LM fusion").  An extension's value is score_add(score_add(s_t(c), g), c == e ? lb : tot), the
// plain one's score_add(s_t(c), ...): alpha = beta = 0 gives the plain bits.  An entry carries its LM state and the unweighted sum of
// its prefix's LM weights; a stay keeps both.  After the last frame, with use_eos, alpha * fin[state] joins every total (fin into
// the LM sum) and the live entries are re-ranked, ties by the previous rank.  Static LDS: the plain 38.5 KiB + 2 x 8 KiB (w, next)
// + 1 KiB of LM state = 55.5 KiB of the 64.
// Lexicon (INTEGRATION.md "Lexicon"): an entry also carries its lexicon node (0.5 KiB more: 56 KiB).  A unit extends along the trie
// with g = 0 -- the plain bits -- and keeps LM state and sum; the space closes the node's word w: g = alpha * lm_step(state, w) +
// beta, the node returns to the root.  After the last frame the entries that do not stand on a word end are dropped, the others
// close their last word (and take alpha * fin with use_eos), and are re-ranked.
// LA (lexicon mode only; INTEGRATION.md "LM look-ahead"): a candidate is ranked by score_add(total, eta), eta = alpha * la[v] + beta
// for the lexicon node v it stands on after the step; the dead test and every carried value stay on the real total.  la[v] of a unit
// extension's child rides in ext_w (which a unit otherwise leaves 0 and nobody reads) and is read per edge (la_edge[e] = la[child_node[e]],
// beside child_node[e]: no hop more in step 0's chain of dependent loads), the root's is one register, an entry's own is loaded beside
// step 0's lookups: 0.25 KiB more LDS, no barrier more.
template <int MODE, bool LA = false>
__device__ __forceinline__ void prefix_beam(const float* __restrict__ sc, int ld, int T, int S, const int* __restrict__ lens, int B, int Cc,
                                            const int* __restrict__ cid_g, const float* __restrict__ csc_g,
                                            const float* __restrict__ sblank_g, LmArgs<MODE> lm, int* __restrict__ tparent,
                                            int* __restrict__ tlabel, int* __restrict__ fnode, int* __restrict__ flen,
                                            float* __restrict__ fscore, int* __restrict__ count, const float* __restrict__ la = nullptr,
                                            const float* __restrict__ la_edge = nullptr) {
  static_assert(!LA || MODE == kLexicon, "the look-ahead ranks along a lexicon");
  __shared__ unsigned long long keys[kMaxKeys];
  __shared__ BeamState st[2];
  __shared__ float stay_lb[kMaxBeam], stay_lnb[kMaxBeam], nx_stay[kMaxBeam], nx_ext[kMaxCls];
  __shared__ int c_id[2][kMaxCls];
  __shared__ float c_sc[2][kMaxCls], c_bl[2];
  __shared__ unsigned long long merged[kMaxBeam];   // per entry: which of its extensions went into another entry's stay
  __shared__ int nb_sh;
  constexpr bool LM = MODE != kPlain, LEX = MODE == kLexicon;
  // the fused search's alone (17 KiB): the plain instantiation never names them, and what is not named is not allocated
  __shared__ int lm_state[2][kMaxBeam];     // the entry's LM state
  __shared__ float lm_sum[2][kMaxBeam];     // ln P_lm of its prefix, unweighted
  __shared__ float ext_w[kMaxKeys / 2];     // this frame's lm_step of (entry p, candidate ci) at p * C' + ci
  __shared__ int ext_next[kMaxKeys / 2];
  __shared__ int lex_node[2][kMaxBeam];     // the lexicon mode's alone: the entry's node of the lexicon trie
  __shared__ int done_sh;                   // ... and the number of complete entries at the end (nb_sh is still being read then)
  __shared__ float la_ent[kMaxBeam];        // the look-ahead's alone: la of the entry's lexicon node, this frame
  const int s = blockIdx.x, tid = threadIdx.x, NT = blockDim.x;
  const int n = min(lens[s], T);
  const size_t cap = 1 + (size_t)T * B;
  int* tp = tparent + (size_t)s * cap;
  int* tl = tlabel + (size_t)s * cap;
  if (tid == 0) {
    st[0].lb[0] = 0.f; st[0].lnb[0] = kLogZero; st[0].se[0] = kLogZero;
    st[0].node[0] = 0; st[0].last[0] = -1; st[0].len[0] = 0; st[0].hash[0] = 0;
    if constexpr (LM) { lm_state[0][0] = lm.tab.start; lm_sum[0][0] = 0.f; }
    if constexpr (LEX) lex_node[0][0] = 0;
    nb_sh = 1;
    tp[0] = -1; tl[0] = -1;
    if (n > 0) c_bl[0] = sblank_g[s];
  }
  if (tid < kMaxBeam) merged[tid] = 0;
  if (n > 0 && tid < Cc) {
    c_id[0][tid] = cid_g[(size_t)s * Cc + tid];
    c_sc[0][tid] = csc_g[(size_t)s * Cc + tid];
  }
  __syncthreads();
  float la_root = 0.f;   // a space extension stands on the root
  if constexpr (LA) la_root = la[0];
  int cur = 0;
  for (int t = 0; t < n; ++t) {
    const int nb = nb_sh;
    if (nb == 0) break;   // the beam died (uniform): possible only with is_log input
    const BeamState& a = st[cur];
    BeamState& nx = st[cur ^ 1];
    const int* ci_ = c_id[t & 1];
    const float* cs_ = c_sc[t & 1];
    const float bl = c_bl[t & 1];
    const int n_ext = nb * Cc;
    // extension of entry p by candidate ci (g is named before s_t(c): the compiler's schedule follows, profiles/ctc_decode_lm.md)
    auto ext_value = [&](int p, int ci) -> float {
      const float lb = a.lb[p], lnb = a.lnb[p];
      float g = 0.f;
      if constexpr (LEX) {
        if (ext_next[p * Cc + ci] < 0) return kLogZero;
        if (ci_[ci] == lm.lex.space) g = __fadd_rn(__fmul_rn(lm.alpha, ext_w[p * Cc + ci]), lm.beta);
      } else if constexpr (LM) g = __fadd_rn(__fmul_rn(lm.alpha, ext_w[p * Cc + ci]), lm.beta);
      const float cs = LM ? score_add(cs_[ci], g) : cs_[ci];
      return score_add(cs, ci_[ci] == a.last[p] ? lb : log_add(lb, lnb));
    };
    // in flight over the whole frame: frame t + 1 (the last frame re-reads itself, unused)
    const size_t row1 = (size_t)min(t + 1, n - 1) * S + s;
    int pf_id = 0;
    float pf_sc = 0.f, pf_ext = 0.f, pf_stay = kLogZero, pf_bl = 0.f;
    if (tid < Cc) {
      pf_id = cid_g[row1 * Cc + tid];
      pf_sc = csc_g[row1 * Cc + tid];
      pf_ext = sc[row1 * ld + ci_[tid]];
    }
    if (tid < nb && a.last[tid] >= 0) pf_stay = sc[row1 * ld + a.last[tid]];
    if (tid == 0) pf_bl = sblank_g[row1];

    if constexpr (LM) {   // ---- 0
      for (int x = tid; x < n_ext; x += NT) {
        const int p = x / Cc, ci = x - p * Cc;
        float w = 0.f;
        int next = -1;
        if constexpr (LEX) {
          const int4 r = reinterpret_cast<const int4*>(lm.lex.node_rec)[lex_node[cur][p]];   // {first child, count, word, 0}
          const int c = ci_[ci];
          if (c != lm.lex.space) {
            const int end = r.x + r.y;
            const int lo = lower_bound(lm.lex.child_cls, r.x, end, c);
            if (lo < end && lm.lex.child_cls[lo] == c) {
              next = lm.lex.child_node[lo];
              if constexpr (LA) w = la_edge[lo];
            }
          } else if (r.z != 0) {
            next = 0;
            if (lm.have_lm) lm_step(lm.tab, lm_state[cur][p], r.z, w, next);
          }
        } else {
          lm_step(lm.tab, lm_state[cur][p], ci_[ci], w, next);
        }
        ext_w[x] = w;
        ext_next[x] = next;
      }
      if constexpr (LA) { if (tid < nb) la_ent[tid] = la[lex_node[cur][tid]]; }
      __syncthreads();
    }
    if (tid < nb) {   // ---- 1
      const int q = tid, e = a.last[q];
      const float lb = a.lb[q], lnb = a.lnb[q];
      const float slb = score_add(bl, log_add(lb, lnb));
      float slnb = e >= 0 ? score_add(a.se[q], lnb) : kLogZero;
      if (e >= 0) {
        const unsigned long long ph = (a.hash[q] - (unsigned long long)(e + 1)) * kHashMulInv;
        const int plen = a.len[q] - 1;
        int p = -1;
        for (int i = 0; i < nb; ++i)
          if (a.hash[i] == ph && a.len[i] == plen) p = i;
        if (p >= 0) {
          const int lo = lower_bound(ci_, 0, Cc, e);
          if (lo < Cc && ci_[lo] == e) {
            slnb = log_add(slnb, ext_value(p, lo));
            atomicOr(&merged[p], 1ull << lo);
          }
        }
      }
      stay_lb[q] = slb;
      stay_lnb[q] = slnb;
      const float total = log_add(slb, slnb) + 0.f;   // (+ 0: a -0 orders as +0)
      float rank = total;
      if constexpr (LA) rank = score_add(total, eta_of(lm.alpha, lm.beta, la_ent[q])) + 0.f;
      keys[q] = total > kDead ? make_key(rank, q) : kDeadKey;
    }
    __syncthreads();
    int npad = 2;   // ---- 2
    while (npad < nb + n_ext) npad <<= 1;   // <= 64 + 2048 -> <= 4096
    for (int x = tid; x < npad - nb; x += NT) {
      unsigned long long key = kDeadKey;
      if (x < n_ext) {
        const int p = x / Cc, ci = x - p * Cc;
        const float v = ext_value(p, ci) + 0.f;
        float rank = v;
        if constexpr (LA) rank = score_add(v, eta_of(lm.alpha, lm.beta, ci_[ci] == lm.lex.space ? la_root : ext_w[x])) + 0.f;
        if (!((merged[p] >> ci) & 1) && v > kDead) key = make_key(rank, kMaxBeam + x);
      }
      keys[nb + x] = key;
    }
    __syncthreads();
    bool first = true;   // ---- 3
    for (int k = 2; k <= npad; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        if (!first) sort_sync(j <= 32);   // the stage before had stride 2 j (<= 64) or 1
        first = false;
        for (int q = tid; q < (npad >> 1); q += NT) {
          const int i = 2 * q - (q & (j - 1)), l = i | j;
          const unsigned long long x = keys[i], y = keys[l];
          if ((x > y) == ((i & k) == 0)) { keys[i] = y; keys[l] = x; }
        }
      }
    // the prefetched frame lands (nothing of it is read before the barrier below; what it replaces was last read before the
    // barrier that ended frame t - 1)
    if (tid < Cc) {
      c_id[(t + 1) & 1][tid] = pf_id;
      c_sc[(t + 1) & 1][tid] = pf_sc;
      nx_ext[tid] = clamp_score(pf_ext);
    }
    if (tid < nb) nx_stay[tid] = clamp_score(pf_stay);
    if (tid == 0) c_bl[(t + 1) & 1] = pf_bl;
    __syncthreads();
    if (tid < 64) {   // ---- 4 (wave 0)
      const unsigned long long key = (tid < B && tid < npad) ? keys[tid] : kDeadKey;
      const bool live = key != kDeadKey;
      if (live) {
        const int idx = (int)(unsigned)key;
        if (idx < kMaxBeam) {
          nx.lb[tid] = stay_lb[idx]; nx.lnb[tid] = stay_lnb[idx]; nx.se[tid] = nx_stay[idx];
          nx.node[tid] = a.node[idx]; nx.last[tid] = a.last[idx]; nx.len[tid] = a.len[idx]; nx.hash[tid] = a.hash[idx];
          if constexpr (LM) { lm_state[cur ^ 1][tid] = lm_state[cur][idx]; lm_sum[cur ^ 1][tid] = lm_sum[cur][idx]; }
          if constexpr (LEX) lex_node[cur ^ 1][tid] = lex_node[cur][idx];
        } else {
          const int x = idx - kMaxBeam, p = x / Cc, ci = x - p * Cc, c = ci_[ci];
          const int node = 1 + t * B + tid;   // < cap: t < n <= T, tid < B
          nx.lb[tid] = kLogZero; nx.lnb[tid] = ext_value(p, ci); nx.se[tid] = nx_ext[ci];
          nx.node[tid] = node; nx.last[tid] = c; nx.len[tid] = a.len[p] + 1;
          nx.hash[tid] = a.hash[p] * kHashMul + (unsigned long long)(c + 1);
          if constexpr (LEX) {   // ext_next is the LM's next state behind a space, the lexicon's child behind a unit
            const bool sp = c == lm.lex.space;
            lex_node[cur ^ 1][tid] = sp ? 0 : ext_next[x];
            lm_state[cur ^ 1][tid] = sp ? ext_next[x] : lm_state[cur][p];
            lm_sum[cur ^ 1][tid] = sp ? __fadd_rn(lm_sum[cur][p], ext_w[x]) : lm_sum[cur][p];
          } else if constexpr (LM) { lm_state[cur ^ 1][tid] = ext_next[x]; lm_sum[cur ^ 1][tid] = __fadd_rn(lm_sum[cur][p], ext_w[x]); }
          tp[node] = a.node[p];
          tl[node] = c;
        }
      }
      const int alive = __popcll(__ballot(live));   // the live keys are a prefix of the sorted array
      if (tid == 0) nb_sh = alive;
      merged[tid] = 0;
    }
    __syncthreads();
    cur ^= 1;
  }
  int nb = nb_sh;
  const BeamState& a = st[cur];
  const size_t out = (size_t)s * B;
  if constexpr (LEX) {
    // the end of the utterance: an entry that stands on a word end closes that word (the empty prefix has none to close), fin
    // joins, the others are dropped, and what is left (<= 64) takes the rank of its new total, ties by the previous rank
    if (tid < kMaxBeam) {   // wave 0
      float total = kLogZero, lsum = kLogZero;
      bool complete = false;
      if (tid < nb) {
        total = log_add(a.lb[tid], a.lnb[tid]) + 0.f;
        lsum = lm_sum[cur][tid];
        int state = lm_state[cur][tid];
        const int w = reinterpret_cast<const int4*>(lm.lex.node_rec)[lex_node[cur][tid]].z;
        complete = a.len[tid] == 0 || w != 0;
        if (complete && a.len[tid] != 0) {
          float wt = 0.f;
          int next = state;
          if (lm.have_lm) lm_step(lm.tab, state, w, wt, next);
          state = next;
          total = clamp_score(__fadd_rn(total, __fadd_rn(__fmul_rn(lm.alpha, wt), lm.beta))) + 0.f;
          lsum = __fadd_rn(lsum, wt);
        }
        if (complete && lm.use_eos) {
          const float f = lm.tab.fin[state];
          total = clamp_score(__fadd_rn(total, __fmul_rn(lm.alpha, f))) + 0.f;
          lsum = __fadd_rn(lsum, f);
        }
      }
      keys[tid] = complete ? make_key(total, tid) : kDeadKey;
      stay_lb[tid] = total;
      stay_lnb[tid] = lsum;
      const int done = __popcll(__ballot(complete));
      if (tid == 0) done_sh = done;
    }
    __syncthreads();
    const int done = done_sh;
    if (tid < B) {
      if (tid < nb && keys[tid] != kDeadKey) {
        int rank = 0;
        for (int i = 0; i < nb; ++i) rank += keys[i] < keys[tid];   // (a dead key is above every live one)
        fnode[out + rank] = a.node[tid];
        flen[out + rank] = a.len[tid];
        fscore[out + rank] = stay_lb[tid];
        lm.flm[out + rank] = stay_lnb[tid];
      }
      if (tid >= done) {
        fnode[out + tid] = -1;
        flen[out + tid] = -1;
        fscore[out + tid] = kLogZero;
        lm.flm[out + tid] = kLogZero;
      }
    }
    nb = done;
  } else if constexpr (!LM) {
    if (tid < B) {
      const bool live = tid < nb;
      fnode[out + tid] = live ? a.node[tid] : -1;
      flen[out + tid] = live ? a.len[tid] : -1;
      fscore[out + tid] = live ? log_add(a.lb[tid], a.lnb[tid]) + 0.f : kLogZero;
    }
  } else {
    // the end of the utterance: fin joins, and the live entries (<= 64, best first) take the rank of their new total
    if (tid < kMaxBeam) {
      float total = kLogZero, lsum = kLogZero;
      if (tid < nb) {
        total = log_add(a.lb[tid], a.lnb[tid]) + 0.f;
        lsum = lm_sum[cur][tid];
        if (lm.use_eos) {
          const float f = lm.tab.fin[lm_state[cur][tid]];
          total = clamp_score(__fadd_rn(total, __fmul_rn(lm.alpha, f))) + 0.f;
          lsum = __fadd_rn(lsum, f);
        }
        keys[tid] = make_key(total, tid);
      }
      stay_lb[tid] = total;
      stay_lnb[tid] = lsum;
    }
    __syncthreads();
    if (tid < B) {
      if (tid < nb) {
        int rank = tid;
        if (lm.use_eos) {
          rank = 0;
          for (int i = 0; i < nb; ++i) rank += keys[i] < keys[tid];
        }
        fnode[out + rank] = a.node[tid];
        flen[out + rank] = a.len[tid];
        fscore[out + rank] = stay_lb[tid];
        lm.flm[out + rank] = stay_lnb[tid];
      } else {
        fnode[out + tid] = -1;
        flen[out + tid] = -1;
        fscore[out + tid] = kLogZero;
        lm.flm[out + tid] = kLogZero;
      }
    }
  }
  if (tid == 0) count[s] = nb;
}

// The kernels of the one text above: <false> the plain search and <true> the token-LM one, as they were named before the text had
// a third mode, and the lexicon search.
template <bool LM>
__global__ __launch_bounds__(512) void ctc_prefix_beam_kernel(const float* __restrict__ sc, int ld, int T, int S,
                                                              const int* __restrict__ lens, int B, int Cc,
                                                              const int* __restrict__ cid_g, const float* __restrict__ csc_g,
                                                              const float* __restrict__ sblank_g, LmArgs<LM ? kTokenLm : kPlain> lm,
                                                              int* __restrict__ tparent, int* __restrict__ tlabel,
                                                              int* __restrict__ fnode, int* __restrict__ flen,
                                                              float* __restrict__ fscore, int* __restrict__ count) {
  prefix_beam<LM ? kTokenLm : kPlain>(sc, ld, T, S, lens, B, Cc, cid_g, csc_g, sblank_g, lm, tparent, tlabel, fnode, flen, fscore, count);
}
__global__ __launch_bounds__(512) void ctc_prefix_beam_lex_kernel(const float* __restrict__ sc, int ld, int T, int S,
                                                                  const int* __restrict__ lens, int B, int Cc,
                                                                  const int* __restrict__ cid_g, const float* __restrict__ csc_g,
                                                                  const float* __restrict__ sblank_g, LmArgs<kLexicon> lm,
                                                                  int* __restrict__ tparent, int* __restrict__ tlabel,
                                                                  int* __restrict__ fnode, int* __restrict__ flen,
                                                                  float* __restrict__ fscore, int* __restrict__ count) {
  prefix_beam<kLexicon>(sc, ld, T, S, lens, B, Cc, cid_g, csc_g, sblank_g, lm, tparent, tlabel, fnode, flen, fscore, count);
}
// ... ranked with the unigram look-ahead la [nodes] (the lexicon's and the word LM's: Lexicon::lookahead)
__global__ __launch_bounds__(512) void ctc_prefix_beam_lex_la_kernel(const float* __restrict__ sc, int ld, int T, int S,
                                                                     const int* __restrict__ lens, int B, int Cc,
                                                                     const int* __restrict__ cid_g, const float* __restrict__ csc_g,
                                                                     const float* __restrict__ sblank_g, LmArgs<kLexicon> lm,
                                                                     const float* __restrict__ la, const float* __restrict__ la_edge,
                                                                     int* __restrict__ tparent,
                                                                     int* __restrict__ tlabel, int* __restrict__ fnode, int* __restrict__ flen,
                                                                     float* __restrict__ fscore, int* __restrict__ count) {
  prefix_beam<kLexicon, true>(sc, ld, T, S, lens, B, Cc, cid_g, csc_g, sblank_g, lm, tparent, tlabel, fnode, flen, fscore, count, la, la_edge);
}

// ---- hypotheses: one lane per (utterance, rank); with an LM (flm, lm_out not null) the lane also hands out its entry's LM sum ------
__global__ __launch_bounds__(64) void ctc_hyp_kernel(const int* __restrict__ tparent, const int* __restrict__ tlabel,
                                                     const int* __restrict__ fnode, const int* __restrict__ flen,
                                                     const float* __restrict__ fscore, const float* __restrict__ flm,
                                                     const int* __restrict__ count, int T, int S, int B, int N, int* __restrict__ hyp,
                                                     int* __restrict__ hyp_len, float* __restrict__ score, float* __restrict__ lm_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S * N) return;
  const int s = i / N, r = i - s * N;
  const int cap = 1 + T * B;
  const int* tp = tparent + (size_t)s * cap;
  const int* tl = tlabel + (size_t)s * cap;
  int* h = hyp + (size_t)i * T;
  const bool have = r < count[s];
  int node = have ? fnode[(size_t)s * B + r] : 0;
  const int L = have ? min(flen[(size_t)s * B + r], T) : 0;
  for (int j = L; j < T; ++j) h[j] = -1;
  for (int j = L - 1; j >= 0 && node > 0 && node < cap; --j) {   // the root is node 0
    h[j] = tl[node];
    node = tp[node];
  }
  hyp_len[i] = have ? L : -1;
  score[i] = have ? fscore[(size_t)s * B + r] : kLogZero;
  if (lm_out) lm_out[i] = have ? flm[(size_t)s * B + r] : kLogZero;
}

// ---- the word beam: lexicons without a boundary unit ----------------------------------------------------------------------------
// INTEGRATION.md "Words without a boundary unit", restated in tests/ctc_words_restatement.py.  A sibling of prefix_beam, not a fourth
// mode of it: an entry has 1 + |words(v)| successors per candidate class, so the successor index, the merge and the end of the
// utterance are all different, and the three instantiations above stay as they are.
struct WordBeamState {
  float lb[kMaxBeam], lnb[kMaxBeam], lmsum[kMaxBeam];
  int node[kMaxBeam], last[kMaxBeam];          // trie node, last label (-1: the empty hypothesis)
  int len[kMaxBeam], nlab[kMaxBeam], nwords[kMaxBeam];   // augmented length (labels + marks), labels, marks
  int closed[kMaxBeam];                        // the word the last step closed in front of its label, or 0
  int lexnode[kMaxBeam], lmstate[kMaxBeam];
  unsigned long long hash[kMaxBeam];           // fingerprint of the augmented sequence: h * M + c + 1 for a label, h * M + K + w for a mark
};
constexpr int kHomStride = 16;   // (entry, word-of-its-node) pairs live at p * 16 + i: Lexicon::kMaxHomophones = 15 < 16
static_assert(Lexicon::kMaxHomophones < kHomStride, "a word index is four bits");

// keys[0, npad), npad a power of two >= 2: ascending, by every thread of the workgroup; the caller's barrier stands before and after
__device__ __forceinline__ void bitonic_sort(unsigned long long* keys, int npad, int tid, int NT) {
  bool first = true;
  for (int k = 2; k <= npad; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (!first) sort_sync(j <= 32);   // the stage before had stride 2 j (<= 64) or 1
      first = false;
      for (int q = tid; q < (npad >> 1); q += NT) {
        const int i = 2 * q - (q & (j - 1)), l = i | j;
        const unsigned long long x = keys[i], y = keys[l];
        if ((x > y) == ((i & k) == 0)) { keys[i] = y; keys[l] = x; }
      }
    }
}

// Grid (S), 64 .. 512 threads.  Successor x = (p * C' + ci) * (1 + H) + slot of entry p, candidate ci: slot 0 stays inside the word
// (the child of p's lexicon node), slot 1 + i closes the i-th word of the node and enters the root's child.  Frame t, between
// workgroup barriers:
//   0  the frame's candidates and the root's child for each (C' lookups); the inside child of every (entry, candidate) (nb * C'
//      bisections); (wt, next) = lm_step of every (entry, word of its node) (at most nb * H walks) -- nothing is looked up after this
//   2  every successor writes its key behind the stays' places; the key array is padded with dead keys to a power of two
//   1  entry q < nb: its stay; the successor that spells q (its parent found by fingerprint: one or two steps back, by whether q's
//      last step closed a word) is log-added into it and its key is struck out -- no bitmask: a successor merges into one entry
//   3  bitonic sort
//   4  rank r < B takes key r: a stay copies its entry, a successor becomes trie node 1 + t * B + r, whose label and closed word
//      are written beside its parent
// Tie index: stays by previous rank, then 64 + x: parent's rank, class id, slot.  After the last frame every complete entry yields
// one final hypothesis per word of its node (key index p * 16 + i), which are sorted and the best B written out.
// Static LDS: 32 KiB keys + 6.5 KiB state + 8 KiB inside children + 12 KiB (wt, next, word) + 1.5 KiB = 60 KiB.
// LA (INTEGRATION.md "LM look-ahead"): a key holds score_add(total, eta), eta = alpha * la[v] + beta for the lexicon node v the
// candidate stands on after the step -- step 4 recomputes every value from (p, ci, slot) and never decodes a key.  la of the root's
// child per candidate and of every entry's own node are step 0's (0.5 KiB more LDS); an inside successor reads la[in_next] from
// global memory where its key is written.
// One text, two kernels (ctc_word_beam.inc): ctc_word_beam_kernel, and ctc_word_beam_la_kernel ranked with the unigram look-ahead.
#define WORD_BEAM_KERNEL ctc_word_beam_kernel
#define WORD_BEAM_LA 0
#include "ctc_word_beam.inc"
#undef WORD_BEAM_KERNEL
#undef WORD_BEAM_LA
#define WORD_BEAM_KERNEL ctc_word_beam_la_kernel
#define WORD_BEAM_LA 1
#include "ctc_word_beam.inc"
#undef WORD_BEAM_KERNEL
#undef WORD_BEAM_LA

// one lane per (utterance, rank): labels, words and word ends out of the trie, back to front
__global__ __launch_bounds__(64) void ctc_word_hyp_kernel(const int* __restrict__ tparent, const int* __restrict__ tlabel,
                                                          const int* __restrict__ tword, const int* __restrict__ fnode,
                                                          const int* __restrict__ flen, const float* __restrict__ fscore,
                                                          const float* __restrict__ flm, const int* __restrict__ fword,
                                                          const int* __restrict__ fnw, const int* __restrict__ count, int T, int S, int B, int N,
                                                          int* __restrict__ hyp, int* __restrict__ hyp_len, float* __restrict__ score,
                                                          float* __restrict__ lm_out, int* __restrict__ words, int* __restrict__ ends,
                                                          int* __restrict__ word_len) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S * N) return;
  const int s = i / N, r = i - s * N;
  const int cap = 1 + T * B;
  const int* tp = tparent + (size_t)s * cap;
  const int* tl = tlabel + (size_t)s * cap;
  const int* tw = tword + (size_t)s * cap;
  int* h = hyp + (size_t)i * T;
  int* wd = words + (size_t)i * T;
  int* en = ends + (size_t)i * T;
  const bool have = r < count[s];
  const size_t f = (size_t)s * B + r;
  int node = have ? fnode[f] : 0;
  const int L = have ? min(flen[f], T) : 0;
  const int W = have ? min(fnw[f], L) : 0;   // every word has a label
  for (int j = 0; j < T; ++j) { h[j] = -1; wd[j] = -1; en[j] = -1; }
  int at = W - 1;
  if (at >= 0) { wd[at] = fword[f]; en[at] = L; --at; }
  for (int j = L - 1; j >= 0 && node > 0 && node < cap; --j) {   // the root is node 0
    h[j] = tl[node];
    const int w = tw[node];   // closed in front of label j: the word ends with label j - 1
    if (w != 0 && at >= 0) { wd[at] = w; en[at] = j; --at; }
    node = tp[node];
  }
  hyp_len[i] = have ? L : -1;
  word_len[i] = have ? W : -1;
  score[i] = have ? fscore[f] : kLogZero;
  lm_out[i] = have ? flm[f] : kLogZero;
}

// The lattices of the returned hypotheses (INTEGRATION.md "Time stamps and CTM"): one workgroup per (utterance, rank) expands the
// labels the hypothesis kernels left on the device -- no host round trip between the search and the alignment of its results.
__global__ __launch_bounds__(256) void ctc_hyp_lattices_kernel(const int* __restrict__ hyp, const int* __restrict__ hyp_len,
                                                               const int* __restrict__ lens, int T, int N, int Lpad,
                                                               int* __restrict__ labx, int* __restrict__ lablens, int* __restrict__ lat_lens,
                                                               int* __restrict__ utt) {
  const int i = blockIdx.x;
  const int U = hyp_len[i];
  // utt != null: the lattices of the scoring sweep (ctc_score), where the empty hypothesis is a lattice of its own -- one blank
  // position over the utterance's frames -- and an entry without a lattice is marked by lablens = 0
  const bool scoring = utt != nullptr;
  const bool have = U >= (scoring ? 0 : 1) && U <= T && 2 * U + 1 <= Lpad;   // (U <= T: a label needs a frame; the hypothesis rows hold T labels)
  const int ll = have ? 2 * U + 1 : 0;
  const int* h = hyp + (size_t)i * T;
  int* lx = labx + (size_t)i * Lpad;
  for (int j = threadIdx.x; j < Lpad; j += blockDim.x) lx[j] = j < ll ? ((j & 1) ? h[j >> 1] : 0) : -1;
  if (threadIdx.x == 0) {
    lablens[i] = have ? ll : scoring ? 0 : 1;
    lat_lens[i] = have ? lens[i / N] : 0;
    if (scoring) utt[i] = i / N;
  }
}

}  // namespace

void ctc_hyp_lattices(hipStream_t st, const int* hyp, const int* hyp_len, const int* lens, int T, int NL, int N, int Lpad, int* labx,
                      int* lablens, int* lat_lens, int* utt) {
  if (NL <= 0) return;
  hipLaunchKernelGGL(ctc_hyp_lattices_kernel, dim3(NL), dim3(256), 0, st, hyp, hyp_len, lens, T, N, Lpad, labx, lablens, lat_lens, utt);
  check_launch("ctc_hyp_lattices");
}

void ctc_row_topc(hipStream_t st, const float* scores, int ld, int rows, int K, int S, const int* lens, int Cc, int* cid, float* csc,
                  float* sblank) {
  if (rows <= 0) return;
  if (K <= 256) hipLaunchKernelGGL(ctc_row_topc_kernel<true>, dim3(cdiv(rows, 4)), dim3(256), 0, st, scores, ld, rows, K, S, lens, Cc, cid, csc, sblank);
  else hipLaunchKernelGGL(ctc_row_topc_kernel<false>, dim3(cdiv(rows, 4)), dim3(256), 0, st, scores, ld, rows, K, S, lens, Cc, cid, csc, sblank);
  check_launch("ctc_row_topc");
}

void ctc_prefix_beam(hipStream_t st, const float* scores, int ld, int T, int S, const int* lens, int B, int Cc, const int* cid,
                     const float* csc, const float* sblank, const LmTables* lm, const LexTables* lex, const float* la, const float* la_edge,
                     float alpha, float beta, bool use_eos, int* tparent, int* tlabel, int* fnode, int* flen, float* fscore, float* flm, int* count) {
  EESEN_REQUIRE(la == nullptr || (lex != nullptr && lm != nullptr && la_edge != nullptr), EESEN_ERR_INVALID, "ctc_prefix_beam: the look-ahead table needs the lexicon and the word LM");
  EESEN_REQUIRE(B >= 1 && B <= kMaxBeam && Cc >= 1 && Cc <= kMaxCls && B * Cc <= kMaxKeys / 2, EESEN_ERR_INVALID, "ctc_prefix_beam: beam or class count outside the key array");
  // one thread per pair of the widest sort stage, 64 .. 512
  int keys = 2;
  while (keys < B + B * Cc) keys <<= 1;
  const int threads = std::min(512, std::max(64, keys / 2));
  if (la) hipLaunchKernelGGL(ctc_prefix_beam_lex_la_kernel, dim3(S), dim3(threads), 0, st, scores, ld, T, S, lens, B, Cc, cid, csc, sblank,
                             LmArgs<kLexicon>{*lm, alpha, beta, use_eos ? 1 : 0, flm, *lex, 1}, la, la_edge, tparent, tlabel, fnode, flen, fscore, count);
  else if (lex) hipLaunchKernelGGL(ctc_prefix_beam_lex_kernel, dim3(S), dim3(threads), 0, st, scores, ld, T, S, lens, B, Cc, cid, csc, sblank,
                              LmArgs<kLexicon>{lm ? *lm : LmTables{}, alpha, beta, use_eos ? 1 : 0, flm, *lex, lm ? 1 : 0}, tparent, tlabel, fnode,
                              flen, fscore, count);
  else if (lm) hipLaunchKernelGGL(ctc_prefix_beam_kernel<true>, dim3(S), dim3(threads), 0, st, scores, ld, T, S, lens, B, Cc, cid, csc, sblank,
                                  LmArgs<kTokenLm>{*lm, alpha, beta, use_eos ? 1 : 0, flm}, tparent, tlabel, fnode, flen, fscore, count);
  else hipLaunchKernelGGL(ctc_prefix_beam_kernel<false>, dim3(S), dim3(threads), 0, st, scores, ld, T, S, lens, B, Cc, cid, csc, sblank,
                          LmArgs<kPlain>{}, tparent, tlabel, fnode, flen, fscore, count);
  check_launch("ctc_prefix_beam");
}

void ctc_hyp(hipStream_t st, const int* tparent, const int* tlabel, const int* fnode, const int* flen, const float* fscore, const float* flm,
             const int* count, int T, int S, int B, int N, int* hyp, int* hyp_len, float* score, float* lm_out) {
  hipLaunchKernelGGL(ctc_hyp_kernel, dim3(cdiv(S * N, 64)), dim3(64), 0, st, tparent, tlabel, fnode, flen, fscore, flm, count, T, S, B, N, hyp, hyp_len,
                     score, lm_out);
  check_launch("ctc_hyp");
}

void ctc_word_beam(hipStream_t st, const float* scores, int ld, int T, int S, const int* lens, int B, int Cc, const int* cid, const float* csc,
                   const float* sblank, const LmTables* lm, const WordLexTables& lex, const float* la, float alpha, float beta, bool use_eos,
                   int* tparent, int* tlabel, int* tword, int* fnode, int* flen, float* fscore, float* flm, int* fword, int* fnw, int* count) {
  EESEN_REQUIRE(la == nullptr || lm != nullptr, EESEN_ERR_INVALID, "ctc_word_beam: the look-ahead table needs the word LM");
  EESEN_REQUIRE(B >= 1 && B <= kMaxBeam && Cc >= 1 && Cc <= kMaxCls && lex.H >= 1 && lex.H <= Lexicon::kMaxHomophones &&
                    B * (1 + Cc * (1 + lex.H)) <= kMaxKeys,
                EESEN_ERR_INVALID, "ctc_word_beam: beam, class count or homophone count outside the key array");
  int keys = 2;
  while (keys < B * (1 + Cc * (1 + lex.H))) keys <<= 1;
  const int threads = std::min(512, std::max(64, keys / 2));
  if (la) hipLaunchKernelGGL(ctc_word_beam_la_kernel, dim3(S), dim3(threads), 0, st, scores, ld, T, S, lens, B, Cc, cid, csc, sblank, *lm, 1, alpha, beta,
                             use_eos ? 1 : 0, lex, la, tparent, tlabel, tword, fnode, flen, fscore, flm, fword, fnw, count);
  else hipLaunchKernelGGL(ctc_word_beam_kernel, dim3(S), dim3(threads), 0, st, scores, ld, T, S, lens, B, Cc, cid, csc, sblank, lm ? *lm : LmTables{},
                          lm ? 1 : 0, alpha, beta, use_eos ? 1 : 0, lex, tparent, tlabel, tword, fnode, flen, fscore, flm, fword, fnw, count);
  check_launch("ctc_word_beam");
}

void ctc_word_hyp(hipStream_t st, const int* tparent, const int* tlabel, const int* tword, const int* fnode, const int* flen, const float* fscore,
                  const float* flm, const int* fword, const int* fnw, const int* count, int T, int S, int B, int N, int* hyp, int* hyp_len,
                  float* score, float* lm_out, int* words, int* ends, int* word_len) {
  hipLaunchKernelGGL(ctc_word_hyp_kernel, dim3(cdiv(S * N, 64)), dim3(64), 0, st, tparent, tlabel, tword, fnode, flen, fscore, flm, fword, fnw, count,
                     T, S, B, N, hyp, hyp_len, score, lm_out, words, ends, word_len);
  check_launch("ctc_word_hyp");
}

}  // namespace eesen
