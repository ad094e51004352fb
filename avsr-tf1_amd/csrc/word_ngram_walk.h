// The model's side of a WORD-level back-off n-gram behind a lexicon trie (include/avsr_hip.h avsr_ctc_prefix_word_ngram describes the
// tables; the rule, with its table of cases, is INTEGRATION.md section 8), shared by the CTC prefix search's word step
// (csrc/ctc_prefix_word_ngram.hip) and beam search's (csrc/beam_word_ngram.hip): ONE copy, so both produce the same bits.
// The state of a label sequence is (h, p): h the automaton node of the words closed so far (walked by csrc/ngram_walk.h, word ids in the
// place of unit ids), p the trie node of the letters since the last space (0 = root, WN_OOV once they have left every spelling).  Three
// scalars are cached with it: close (what a space costs), hc (the node that space leaves; h at the root) and eos = close +
// walk(hc, </s>).  fp32 additions in this fixed order, plain loads.  Nothing here can run away on tables it was not meant for: the walk
// is bounded and clamped (ngram_walk.h), the trie search is the same clamped binary search, and every node and word id read from a
// table is clamped into its table before it is used as an index.
#pragma once
#include "ngram_walk.h"

namespace avsr {

#define WN_FLOOR (-227.95592420641054f)                                     // -99 ln 10 (ngram.FLOOR), rounded to fp32 once
#define WN_OOV (-1)

// the lexicon trie: CSR over nodes, children sorted by unit id
struct trie_view {
  int n_nodes, n_arcs;
  const int32_t* begin; const int32_t* sym; const int32_t* next; const int32_t* word;
};

// the child of trie node p (0 <= p < n_nodes) under unit c, or WN_OOV
__device__ __forceinline__ int trie_child(const trie_view& T, int p, int c) {
  int lo = T.begin[p], end = T.begin[p + 1];
  lo = lo < 0 ? 0 : lo;
  end = end > T.n_arcs ? T.n_arcs : end;
  int hi = end;
  while (lo < hi) {                                                        // the first child with sym >= c
    const int mid = (lo + hi) >> 1;
    if (T.sym[mid] < c) lo = mid + 1; else hi = mid;
  }
  if (!(lo < end && T.sym[lo] == c)) return WN_OOV;
  const int n = T.next[lo];
  return (unsigned)n < (unsigned)T.n_nodes ? n : WN_OOV;
}

// the two tables and the scalars of a word model (the descriptors of both steps carry these fields under these names)
struct word_model {
  const ngram_view G;
  const trie_view T;
  const int V, Vw, start, eos_w, unk_id, space_id, go_id, eos_id;
  const float oov;
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
  // (h, p) of g . c from the parent's (h, p, hc): a space takes the cached hc, EOS one walk from it, a letter one search among the trie
  // node's children (at most one trie search or one walk); MASK and GO leave the state as it is
  __device__ __forceinline__ void advance(int& h, int& p, int hc, int c) const {
    if (c == space_id) { h = hc; p = 0; }                                  // (at the root hc = h)
    else if (c == eos_id) {
      int arc;
      ngram_walk(G, hc, eos_w, arc);
      h = ngram_node(G, G.next[arc]); p = 0;
    } else if (c != go_id && c != 0) {
      if (p >= 0) p = trie_child(T, p, c);
    }
  }
  // close / hc / eos of the state (h, p): at most two dependent walks
  __device__ __forceinline__ void scalars(int h, int p, float& cl, int& hc, float& eos) const {
    int arc;
    cl = 0.f;
    hc = h;
    if (p != 0) cl = close(h, p, hc);
    eos = cl + ngram_walk(G, hc, eos_w, arc);
  }
  // lam(c | g) at a state with trie node p and the scalars cl, eos: a letter is one search among the children of p (0 if found or at
  // OOV, else oov); space, EOS and the non-units (class 0 = MASK, GO: the floor) come from the scalars
  __device__ __forceinline__ float value(int p, int c, float cl, float eos) const {
    if (c == space_id) return cl;
    if (c == eos_id) return eos;
    if (c == go_id || c == 0) return WN_FLOOR;
    return (p < 0 || trie_child(T, p, c) >= 0) ? 0.f : oov;
  }
};

template <class Desc>
__host__ __device__ __forceinline__ word_model word_model_of(const Desc& d) {
  return word_model{ngram_view_of(d), trie_view{d.n_trie_nodes, d.n_trie_arcs, d.t_begin, d.t_sym, d.t_next, d.t_word},
                    d.V, d.Vw, d.start, d.eos_w, d.unk_id, d.space_id, d.go_id, d.eos_id, d.oov};
}

}  // namespace avsr
