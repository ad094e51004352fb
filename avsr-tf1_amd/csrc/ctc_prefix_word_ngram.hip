// CTC prefix beam search over CHARACTERS with a WORD-level back-off n-gram fused into the frame loop through a lexicon trie
// (avsr_ctc_prefix_search_word_ngram, include/avsr_hip.h; the rule is INTEGRATION.md section 8): the search of csrc/ctc_prefix_search.h
// (cp_search: ONE launch per batch, one 256-thread workgroup per utterance, the beam in LDS, fp32, no atomics, two launches
// bit-identical) with lam(. | g) formed from two device-resident read-only tables -- the word automaton, walked by csrc/ngram_walk.h as
// it is (word ids in the place of unit ids), and the trie over the vocabulary's spellings.  The model's side -- the trie search, the
// transition, close / hc / eos and the per-class value -- is csrc/word_ngram_walk.h, one copy shared with beam search's word step
// (csrc/beam_word_ngram.hip); this file places its state in the search's LDS.
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
#include "word_ngram_walk.h"

namespace avsr {

// the word model (word_ngram_walk.h) as cp_search's Step: five words per pool row in LDS
struct cpw_step {
  const word_model M;
  int* sH; int* sP; float* sClose; int* sHc; float* sEos;                  // [2 W] each
  static size_t extra(int W) { return 10 * (size_t)W; }
  __device__ __forceinline__ void init(int, int W, uint32_t* words) {
    sH = reinterpret_cast<int*>(words); sP = sH + 2 * W; sClose = reinterpret_cast<float*>(sP + 2 * W);
    sHc = reinterpret_cast<int*>(sClose + 2 * W); sEos = reinterpret_cast<float*>(sHc + 2 * W);
  }
  __device__ __forceinline__ void prologue(int) {}
  __device__ __forceinline__ void step(int M_, const int* sTok, const int* sPar, const int* sNew, float* sLam, bool first) {
    const int tid = threadIdx.x, V = M.V;
    if (tid < M_) {
      int h = ngram_node(M.G, M.start), p = 0;
      if (!first) {
        const int par = sPar[tid];
        h = sH[par]; p = sP[par];
        M.advance(h, p, sHc[par], sTok[tid]);
      }
      float cl, eos;
      int hc;
      M.scalars(h, p, cl, hc, eos);
      const int nw = sNew[tid];
      sH[nw] = h; sP[nw] = p; sClose[nw] = cl; sHc[nw] = hc; sEos[nw] = eos;
    }
    lds_barrier();
    for (int e = tid; e < M_ * V; e += 256) {
      const int m = e / V, c = e - m * V, nw = sNew[m];
      sLam[nw * V + c] = M.value(sP[nw], c, sClose[nw], sEos[nw]);
    }
    lds_barrier();
  }
};

// dynamic LDS: cp_lds_words(V, W, L_max, true, 10 W) words
__global__ __launch_bounds__(256) void ctc_prefix_word_ngram_kernel(const avsr_ctc_prefix_args A, const avsr_ctc_prefix_word_ngram G) {
  extern __shared__ __attribute__((aligned(16))) uint32_t cpw_smem[];
  cpw_step step{word_model_of(G), nullptr, nullptr, nullptr, nullptr, nullptr};
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
