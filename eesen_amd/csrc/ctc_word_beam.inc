// ctc_word_beam.inc -- the text of the word beam kernel (ctc_decode.hip includes it twice: WORD_BEAM_KERNEL names the kernel,
// WORD_BEAM_LA is 0 for ctc_word_beam_kernel and 1 for ctc_word_beam_la_kernel, which takes the look-ahead table la [nodes]).
__global__ __launch_bounds__(512) void WORD_BEAM_KERNEL(const float* __restrict__ sc, int ld, int T, int S, const int* __restrict__ lens, int B,
                                                        int Cc, const int* __restrict__ cid_g, const float* __restrict__ csc_g,
                                                        const float* __restrict__ sblank_g, LmTables tab, int have_lm, float alpha, float beta,
                                                        int use_eos, WordLexTables lex,
#if WORD_BEAM_LA
                                                        const float* __restrict__ la,
#endif
                                                        int* __restrict__ tparent, int* __restrict__ tlabel,
                                                        int* __restrict__ tword, int* __restrict__ fnode, int* __restrict__ flen,
                                                        float* __restrict__ fscore, float* __restrict__ flm, int* __restrict__ fword,
                                                        int* __restrict__ fnw, int* __restrict__ count) {
  __shared__ unsigned long long keys[kMaxKeys];
#if WORD_BEAM_LA
  __shared__ float la_root[kMaxCls], la_ent[kMaxBeam];   // la of root_next[ci], of the entry's node
#endif
  __shared__ WordBeamState st[2];
  __shared__ float stay_lb[kMaxBeam], stay_lnb[kMaxBeam];
  __shared__ int c_id[kMaxCls], root_next[kMaxCls];
  __shared__ float c_sc[kMaxCls], c_bl;
  __shared__ int in_next[kMaxKeys / 2];                 // the inside child of (p, ci) at p * C' + ci, or -1
  __shared__ float cl_w[kMaxBeam * kHomStride];         // lm_step of (p, i-th word of p's node) at p * 16 + i
  __shared__ int cl_next[kMaxBeam * kHomStride], cl_word[kMaxBeam * kHomStride];
  __shared__ int ent_nw[kMaxBeam];                      // |words(v)| of the entry's node
  __shared__ int nb_sh;
  const int s = blockIdx.x, tid = threadIdx.x, NT = blockDim.x;
  const int n = min(lens[s], T);
  const size_t cap = 1 + (size_t)T * B;
  int* tp = tparent + (size_t)s * cap;
  int* tl = tlabel + (size_t)s * cap;
  int* tw = tword + (size_t)s * cap;
  const int4* __restrict__ nrec = reinterpret_cast<const int4*>(lex.node_rec);   // {first child, child count, first word slot, word count}
  const int H1 = 1 + lex.H;
  if (tid == 0) {
    WordBeamState& z = st[0];
    z.lb[0] = 0.f; z.lnb[0] = kLogZero; z.lmsum[0] = 0.f;
    z.node[0] = 0; z.last[0] = -1; z.len[0] = 0; z.nlab[0] = 0; z.nwords[0] = 0; z.closed[0] = 0; z.lexnode[0] = 0;
    z.lmstate[0] = have_lm ? tab.start : 0; z.hash[0] = 0;
    nb_sh = 1;
    tp[0] = -1; tl[0] = -1; tw[0] = 0;
  }
  __syncthreads();
  int cur = 0;
  for (int t = 0; t < n; ++t) {
    const int nb = nb_sh;
    if (nb == 0) break;   // the beam died (uniform): possible only with is_log input
    const WordBeamState& a = st[cur];
    WordBeamState& nx = st[cur ^ 1];
    const size_t row = (size_t)t * S + s;
    const int* cid_row = cid_g + row * Cc;
    // ---- 0
    if (tid < Cc) {
      const int c = cid_row[tid];
      c_id[tid] = c;
      c_sc[tid] = csc_g[row * Cc + tid];
      const int4 r = nrec[0];
      const int end = r.x + r.y;
      const int lo = lower_bound(lex.child_cls, r.x, end, c);
      root_next[tid] = (lo < end && lex.child_cls[lo] == c) ? lex.child_node[lo] : -1;
#if WORD_BEAM_LA
      la_root[tid] = root_next[tid] >= 0 ? la[root_next[tid]] : 0.f;
#endif
    }
#if WORD_BEAM_LA
    if (tid < nb) la_ent[tid] = la[a.lexnode[tid]];
#endif
    if (tid == 0) c_bl = sblank_g[row];
    for (int x = tid; x < nb * Cc; x += NT) {
      const int p = x / Cc, ci = x - p * Cc;
      const int4 r = nrec[a.lexnode[p]];
      const int c = cid_row[ci];
      const int end = r.x + r.y;
      const int lo = lower_bound(lex.child_cls, r.x, end, c);
      in_next[x] = (lo < end && lex.child_cls[lo] == c) ? lex.child_node[lo] : -1;
    }
    for (int x = tid; x < nb * kHomStride; x += NT) {
      const int p = x / kHomStride, i = x - p * kHomStride;
      const int4 r = nrec[a.lexnode[p]];
      if (i == 0) ent_nw[p] = r.w;
      if (i < r.w) {
        const int w = lex.node_words[r.z + i];
        float wt = 0.f;
        int next = a.lmstate[p];
        if (have_lm) lm_step(tab, a.lmstate[p], w, wt, next);
        cl_w[x] = wt; cl_next[x] = next; cl_word[x] = w;
      }
    }
    __syncthreads();
    const float bl = c_bl;
    auto succ_value = [&](int p, int ci, int slot) -> float {
      float g = 0.f;
      if (slot == 0) {
        if (in_next[p * Cc + ci] < 0) return kLogZero;
      } else {
        if (slot - 1 >= ent_nw[p] || root_next[ci] < 0) return kLogZero;
        g = __fadd_rn(__fmul_rn(alpha, cl_w[p * kHomStride + slot - 1]), beta);
      }
      const float lb = a.lb[p], lnb = a.lnb[p];
      const float cs = score_add(c_sc[ci], g);
      return score_add(cs, c_id[ci] == a.last[p] ? lb : log_add(lb, lnb));
    };
    const int n_succ = nb * Cc * H1;   // nb + n_succ <= B * (1 + C' * (1 + H)) <= kMaxKeys: the host's limit
    int npad = 2;
    while (npad < nb + n_succ) npad <<= 1;
    for (int x = tid; x < npad - nb; x += NT) {   // ---- 2
      unsigned long long key = kDeadKey;
      if (x < n_succ) {
        const int pc = x / H1, slot = x - pc * H1, p = pc / Cc, ci = pc - p * Cc;
        const float v = succ_value(p, ci, slot) + 0.f;
#if WORD_BEAM_LA
        if (v > kDead) key = make_key(score_add(v, eta_of(alpha, beta, slot == 0 ? la[in_next[pc]] : la_root[ci])) + 0.f, kMaxBeam + x);   // (alive: the node exists)
#else
        if (v > kDead) key = make_key(v, kMaxBeam + x);
#endif
      }
      keys[nb + x] = key;
    }
    __syncthreads();
    if (tid < nb) {   // ---- 1
      const int q = tid, e = a.last[q];
      const float lb = a.lb[q], lnb = a.lnb[q];
      const float slb = score_add(bl, log_add(lb, lnb));
      float slnb = kLogZero;
      if (e >= 0) {
        slnb = score_add(clamp_score(sc[row * ld + e]), lnb);
        const int w = a.closed[q];
        unsigned long long ph = (a.hash[q] - (unsigned long long)(e + 1)) * kHashMulInv;
        int plen = a.len[q] - 1;
        if (w != 0) { ph = (ph - (unsigned long long)(lex.K + w)) * kHashMulInv; --plen; }
        int p = -1;
        for (int i = 0; i < nb; ++i)
          if (a.hash[i] == ph && a.len[i] == plen) p = i;
        if (p >= 0) {
          const int lo = lower_bound(c_id, 0, Cc, e);
          if (lo < Cc && c_id[lo] == e) {
            int slot = w == 0 ? 0 : -1;
            for (int i = 0; w != 0 && i < ent_nw[p]; ++i)
              if (cl_word[p * kHomStride + i] == w) slot = 1 + i;
            if (slot >= 0) {
              slnb = log_add(slnb, succ_value(p, lo, slot));
              keys[nb + (p * Cc + lo) * H1 + slot] = kDeadKey;
            }
          }
        }
      }
      stay_lb[q] = slb;
      stay_lnb[q] = slnb;
      const float total = log_add(slb, slnb) + 0.f;   // (+ 0: a -0 orders as +0)
#if WORD_BEAM_LA
      keys[q] = total > kDead ? make_key(score_add(total, eta_of(alpha, beta, la_ent[q])) + 0.f, q) : kDeadKey;
#else
      keys[q] = total > kDead ? make_key(total, q) : kDeadKey;
#endif
    }
    __syncthreads();
    bitonic_sort(keys, npad, tid, NT);   // ---- 3
    __syncthreads();
    if (tid < 64) {   // ---- 4 (wave 0)
      const unsigned long long key = (tid < B && tid < npad) ? keys[tid] : kDeadKey;
      const bool live = key != kDeadKey;
      if (live) {
        const int idx = (int)(unsigned)key;
        if (idx < kMaxBeam) {
          nx.lb[tid] = stay_lb[idx]; nx.lnb[tid] = stay_lnb[idx]; nx.lmsum[tid] = a.lmsum[idx];
          nx.node[tid] = a.node[idx]; nx.last[tid] = a.last[idx]; nx.len[tid] = a.len[idx]; nx.nlab[tid] = a.nlab[idx];
          nx.nwords[tid] = a.nwords[idx]; nx.closed[tid] = a.closed[idx]; nx.lexnode[tid] = a.lexnode[idx];
          nx.lmstate[tid] = a.lmstate[idx]; nx.hash[tid] = a.hash[idx];
        } else {
          const int x = idx - kMaxBeam, pc = x / H1, slot = x - pc * H1, p = pc / Cc, ci = pc - p * Cc, c = c_id[ci];
          const int node = 1 + t * B + tid;   // < cap: t < n <= T, tid < B
          const int at = p * kHomStride + slot - 1;
          const int w = slot == 0 ? 0 : cl_word[at];
          unsigned long long h = a.hash[p];
          if (slot != 0) h = h * kHashMul + (unsigned long long)(lex.K + w);
          nx.lb[tid] = kLogZero; nx.lnb[tid] = succ_value(p, ci, slot);
          nx.lmsum[tid] = slot == 0 ? a.lmsum[p] : __fadd_rn(a.lmsum[p], cl_w[at]);
          nx.node[tid] = node; nx.last[tid] = c;
          nx.len[tid] = a.len[p] + (slot == 0 ? 1 : 2); nx.nlab[tid] = a.nlab[p] + 1; nx.nwords[tid] = a.nwords[p] + (slot == 0 ? 0 : 1);
          nx.closed[tid] = w;
          nx.lexnode[tid] = slot == 0 ? in_next[p * Cc + ci] : root_next[ci];
          nx.lmstate[tid] = slot == 0 ? a.lmstate[p] : cl_next[at];
          nx.hash[tid] = h * kHashMul + (unsigned long long)(c + 1);
          tp[node] = a.node[p];
          tl[node] = c;
          tw[node] = w;
        }
      }
      const int alive = __popcll(__ballot(live));   // the live keys are a prefix of the sorted array
      if (tid == 0) nb_sh = alive;
    }
    __syncthreads();
    cur ^= 1;
  }
  // the end of the utterance: a complete entry yields one final hypothesis per word of its node (the empty one: itself), each closes
  // its word and takes fin with use_eos; they are ranked by the new total, ties by (previous rank, word index)
  const int nb = nb_sh;
  const WordBeamState& a = st[cur];
  float* fin_tot = reinterpret_cast<float*>(in_next);   // [64 * 16]: the frames' use of in_next is over
  int npad = kHomStride;
  while (npad < nb * kHomStride) npad <<= 1;   // <= 1024
  for (int x = tid; x < npad; x += NT) {
    const int p = x / kHomStride, i = x - p * kHomStride;
    unsigned long long key = kDeadKey;
    if (p < nb) {
      const int4 r = nrec[a.lexnode[p]];
      const bool empty = a.len[p] == 0;
      if (empty ? i == 0 : i < r.w) {
        float total = log_add(a.lb[p], a.lnb[p]) + 0.f, lsum = a.lmsum[p];
        int state = a.lmstate[p], w = 0;
        if (!empty) {
          w = lex.node_words[r.z + i];
          float wt = 0.f;
          int next = state;
          if (have_lm) lm_step(tab, state, w, wt, next);
          state = next;
          total = clamp_score(__fadd_rn(total, __fadd_rn(__fmul_rn(alpha, wt), beta))) + 0.f;
          lsum = __fadd_rn(lsum, wt);
        }
        if (use_eos) {
          const float f = tab.fin[state];
          total = clamp_score(__fadd_rn(total, __fmul_rn(alpha, f))) + 0.f;
          lsum = __fadd_rn(lsum, f);
        }
        key = make_key(total, x);
        fin_tot[x] = total; cl_w[x] = lsum; cl_word[x] = w;
      }
    }
    keys[x] = key;
  }
  __syncthreads();
  bitonic_sort(keys, npad, tid, NT);
  __syncthreads();
  if (tid < 64) {   // wave 0; B <= 64
    const unsigned long long key = (tid < B && tid < npad) ? keys[tid] : kDeadKey;
    const bool live = key != kDeadKey;
    if (tid < B) {
      const size_t o = (size_t)s * B + tid;
      const int x = (int)(unsigned)key, p = x / kHomStride;
      fnode[o] = live ? a.node[p] : -1;
      flen[o] = live ? a.nlab[p] : -1;
      fscore[o] = live ? fin_tot[x] : kLogZero;
      flm[o] = live ? cl_w[x] : kLogZero;
      fword[o] = live ? cl_word[x] : -1;
      fnw[o] = live ? a.nwords[p] + (cl_word[x] != 0 ? 1 : 0) : -1;
    }
    const int done = __popcll(__ballot(live));
    if (tid == 0) count[s] = done;
  }
}
