// CTC prefix beam search over CHARACTERS with a WORD-level back-off n-gram fused into the frame loop through a lexicon trie
// (avsr_ctc_prefix_search_word_ngram, include/avsr_hip.h; the rule is INTEGRATION.md section 8): the search of csrc/ctc_prefix_search.h
// (cp_search: ONE launch per batch, one 256-thread workgroup per utterance, the beam in LDS, fp32, no atomics, two launches
// bit-identical) with lam(. | g) formed from two device-resident read-only tables -- the word automaton, walked by csrc/ngram_walk.h as
// it is (word ids in the place of unit ids), and the trie over the vocabulary's spellings.  This file is the model's side only.
//
// State placement.  Per label sequence the model holds FIVE words in LDS behind the search's own, [2 W rows] each, addressed by the
// same per-slot row index as the lam rows (a stay inherits its parent's row, an extension takes a row no old slot references, so no
// step reads a row that the same step writes):
//   h      the automaton node of the words closed so far            p      the trie node of the letters since the last space
//                                                                          (0 = root, -1 = OOV: they have left every spelling)
//   close  what a space costs here (0 at the root)                  hc     the automaton node after that space (h at the root)
//   eos    close + walk(hc, </s>): the row's EOS column
// No workspace, no global-memory state: the only global traffic of a step is the read-only tables.
//
// Phase 6 for the M <= 16 kept extensions of a frame (skipped by the search's workgroup-uniform branch when M = 0):
//   a. thread m < M:  (h, p)[new_m] from (h, p, hc)[parent_m] and tok_m -- a space takes the parent's cached hc, EOS one walk from it,
//      a letter one search among the trie node's children (at most one trie search and one walk); then close / hc / eos of the new row
//      (at most two dependent walks)                                                              (prologue: h = start, p = root)
//   b. M * V entries over the 256 threads: a letter is one search among the children of p (0 if found or at OOV, else oov); space,
//      EOS and the non-units (class 0 = MASK, GO: the floor -99 ln 10) come from the row's scalars.
// Nothing here can run away on tables it was not meant for: the walk is bounded and clamped (ngram_walk.h), the trie search is the same
// clamped binary search, and every node and word id read from a table is clamped into its table before it is used as an index.
#include "ctc_prefix_search.h"
#include "ngram_walk.h"

namespace avsr {

#define CPW_FLOOR (-227.95592420641054f)                                    // -99 ln 10 (ngram.FLOOR), rounded to fp32 once
#define CPW_OOV (-1)

// the lexicon trie: CSR over nodes, children sorted by unit id
struct trie_view {
  int n_nodes, n_arcs;
  const int32_t* begin; const int32_t* sym; const int32_t* next; const int32_t* word;
};

// the child of trie node p (0 <= p < n_nodes) under unit c, or CPW_OOV
__device__ __forceinline__ int trie_child(const trie_view& T, int p, int c) {
  int lo = T.begin[p], end = T.begin[p + 1];
  lo = lo < 0 ? 0 : lo;
  end = end > T.n_arcs ? T.n_arcs : end;
  int hi = end;
  while (lo < hi) {                                                        // the first child with sym >= c
    const int mid = (lo + hi) >> 1;
    if (T.sym[mid] < c) lo = mid + 1; else hi = mid;
  }
  if (!(lo < end && T.sym[lo] == c)) return CPW_OOV;
  const int n = T.next[lo];
  return (unsigned)n < (unsigned)T.n_nodes ? n : CPW_OOV;
}

// the word model behind the trie as cp_search's Step: five words per pool row in LDS
struct cpw_step {
  const ngram_view G;
  const trie_view T;
  const int V, Vw, start, eos_w, unk_id, space_id, go_id, eos_id;
  const float oov;
  int* sH; int* sP; float* sClose; int* sHc; float* sEos;                  // [2 W] each
  static size_t extra(int W) { return 10 * (size_t)W; }
  __device__ __forceinline__ void init(int, int W, uint32_t* words) {
    sH = reinterpret_cast<int*>(words); sP = sH + 2 * W; sClose = reinterpret_cast<float*>(sP + 2 * W);
    sHc = reinterpret_cast<int*>(sClose + 2 * W); sEos = reinterpret_cast<float*>(sHc + 2 * W);
  }
  __device__ __forceinline__ void prologue(int) {}
  __device__ __forceinline__ int word_id(int w) const { return (unsigned)w < (unsigned)Vw ? w : -1; }
  // what a space costs at (h, p != root) and the node it leaves: the word p ends, else <unk> (oov first for a proper prefix)
  __device__ __forceinline__ float close(int h, int p, int& hc) const {
    int w = p > 0 ? word_id(T.word[p]) : -1;
    const bool prefix = p > 0 && w < 0;
    if (w < 0) w = word_id(unk_id);
    float v = 0.f;
    hc = 0;
    if (w >= 0) {
      int arc;
      v = ngram_walk(G, h, w, arc);
      hc = ngram_node(G, G.next[arc]);
    }
    return prefix ? oov + v : v;
  }
  __device__ __forceinline__ void step(int M, const int* sTok, const int* sPar, const int* sNew, float* sLam, bool first) {
    const int tid = threadIdx.x;
    if (tid < M) {
      int h = ngram_node(G, start), p = 0;
      if (!first) {
        const int par = sPar[tid], c = sTok[tid];
        h = sH[par]; p = sP[par];
        if (c == space_id) { h = sHc[par]; p = 0; }                        // (at the root hc = h)
        else if (c == eos_id) {
          int arc;
          ngram_walk(G, sHc[par], eos_w, arc);
          h = ngram_node(G, G.next[arc]); p = 0;
        } else if (c != go_id && c != 0) {
          if (p >= 0) p = trie_child(T, p, c);
        }
      }
      float cl = 0.f;
      int hc = h, arc;
      if (p != 0) cl = close(h, p, hc);
      const int nw = sNew[tid];
      sH[nw] = h; sP[nw] = p; sClose[nw] = cl; sHc[nw] = hc; sEos[nw] = cl + ngram_walk(G, hc, eos_w, arc);
    }
    lds_barrier();
    for (int e = tid; e < M * V; e += 256) {
      const int m = e / V, c = e - m * V, nw = sNew[m], p = sP[nw];
      float v;
      if (c == space_id) v = sClose[nw];
      else if (c == eos_id) v = sEos[nw];
      else if (c == go_id || c == 0) v = CPW_FLOOR;
      else v = (p < 0 || trie_child(T, p, c) >= 0) ? 0.f : oov;
      sLam[nw * V + c] = v;
    }
    lds_barrier();
  }
};

// dynamic LDS: cp_lds_words(V, W, L_max, true, 10 W) words
__global__ __launch_bounds__(256) void ctc_prefix_word_ngram_kernel(const avsr_ctc_prefix_args A, const avsr_ctc_prefix_word_ngram G) {
  extern __shared__ __attribute__((aligned(16))) uint32_t cpw_smem[];
  cpw_step step{ngram_view_of(G), trie_view{G.n_trie_nodes, G.n_trie_arcs, G.t_begin, G.t_sym, G.t_next, G.t_word},
                G.V, G.Vw, G.start, G.eos_w, G.unk_id, G.space_id, G.go_id, G.eos_id, G.oov, nullptr, nullptr, nullptr, nullptr, nullptr};
  const cp_terms terms{G.weight, G.bonus, G.go_id, G.eos_id, G.s_lm, G.lm_steps, G.lm_logp};
  cp_search(A, terms, step, cpw_smem);
}

// AVSR_OK, or why the shape cannot run (decided on the host, nothing dereferenced)
static int ctc_prefix_word_ngram_limits(int V, int W, int LM, int n_nodes, int n_arcs, int Vw, int n_t, int n_ta) {
  const bool bad = n_nodes < 1 || Vw < 2 || n_arcs < Vw || n_t < 1 || n_ta < 1;
  const bool big = n_nodes > AVSR_CTC_PREFIX_NGRAM_MAX_NODES || n_arcs > AVSR_CTC_PREFIX_NGRAM_MAX_ARCS ||
                   n_t > AVSR_CTC_PREFIX_NGRAM_MAX_NODES || n_ta > AVSR_CTC_PREFIX_NGRAM_MAX_ARCS;
  return cp_limits(V, W, LM, AVSR_CTC_PREFIX_LM_MAX_W, true, cpw_step::extra(W), bad, big);
}

}  // namespace avsr

extern "C" int avsr_ctc_prefix_word_ngram_supported(int32_t V, int32_t beam_width, int32_t L_max, int32_t n_nodes, int32_t n_arcs,
                                                    int32_t Vw, int32_t n_trie_nodes, int32_t n_trie_arcs) {
  return avsr::ctc_prefix_word_ngram_limits(V, beam_width, L_max, n_nodes, n_arcs, Vw, n_trie_nodes, n_trie_arcs) == AVSR_OK ? 1 : 0;
}

extern "C" int avsr_ctc_prefix_search_word_ngram(const avsr_ctc_prefix_args* a, const avsr_ctc_prefix_word_ngram* wg, void* stream) {
  using namespace avsr;
  if (!wg) return AVSR_ERR_ARG;
  int rc = cp_check_args(a);
  if (!rc) rc = cp_check_terms(a->V, wg->V, wg->go_id, wg->eos_id, wg->weight, wg->bonus);
  if (!rc) rc = ctc_prefix_word_ngram_limits(a->V, a->beam_width, a->L_max, wg->n_nodes, wg->n_arcs, wg->Vw, wg->n_trie_nodes, wg->n_trie_arcs);
  if (rc) return rc;
  if (wg->start < 0 || wg->start >= wg->n_nodes || wg->eos_w < 0 || wg->eos_w >= wg->Vw || wg->unk_id < -1 || wg->unk_id >= wg->Vw)
    return AVSR_ERR_ARG;
  if (wg->space_id < 0 || wg->space_id >= wg->V || wg->space_id == wg->go_id || wg->space_id == wg->eos_id || wg->go_id == wg->eos_id)
    return AVSR_ERR_ARG;
  if (!(wg->oov <= 0.f) || wg->oov == -INFINITY) return AVSR_ERR_ARG;
  if (!wg->bow || !wg->backoff || !wg->arc_begin || !wg->sym || !wg->logp || !wg->next || !wg->s_lm || !wg->lm_steps) return AVSR_ERR_ARG;
  if (!wg->t_begin || !wg->t_sym || !wg->t_next || !wg->t_word) return AVSR_ERR_ARG;
  const size_t lds = sizeof(uint32_t) * cp_lds_words(a->V, a->beam_width, a->L_max, true, cpw_step::extra(a->beam_width));
  return cp_launch<ctc_prefix_word_ngram_kernel>(lds, stream, *a, *wg);
}
