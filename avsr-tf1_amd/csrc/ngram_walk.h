// The walk over a device-resident back-off n-gram automaton (include/avsr_hip.h avsr_ctc_prefix_ngram describes the six tables; the rule
// is INTEGRATION.md section 8), shared by the CTC prefix search's n-gram step (csrc/ctc_prefix_ngram.hip) and beam search's
// (csrc/beam_ngram.hip): ONE copy, so both produce the same bits.
// One walk: acc = 0; while the node has no arc for c (binary search among its sorted arcs; the ROOT holds all V classes, so there the arc
// is index c): acc += bow[node], node = backoff[node]; then acc + logp[arc].  fp32 additions in this fixed order, plain loads.
// A walk is a chain of dependent L2 reads (arc_begin, ~log2(arcs) probes of sym, bow / backoff per level); the tables are not staged in
// LDS.  It cannot run away on tables it was not meant for: at most AVSR_CTC_PREFIX_NGRAM_MAX_ORDER - 1 nodes are visited before the root
// is read directly, and every node id and arc range is clamped into its table.
#pragma once
#include "common.h"
#include "avsr_hip.h"

namespace avsr {

// the six tables of an automaton (the descriptors of both steps carry these fields under these names)
struct ngram_view {
  int n_nodes, n_arcs;
  const float* bow; const int32_t* backoff; const int32_t* arc_begin;
  const int32_t* sym; const float* logp; const int32_t* next;
};

template <class Desc>
__host__ __device__ __forceinline__ ngram_view ngram_view_of(const Desc& d) {
  return ngram_view{d.n_nodes, d.n_arcs, d.bow, d.backoff, d.arc_begin, d.sym, d.logp, d.next};
}

__device__ __forceinline__ int ngram_node(const ngram_view& G, int n) { return (unsigned)n < (unsigned)G.n_nodes ? n : 0; }

// the arc of class c at node n != 0, or -1
__device__ __forceinline__ int ngram_find(const ngram_view& G, int n, int c) {
  int lo = G.arc_begin[n], end = G.arc_begin[n + 1];
  lo = lo < 0 ? 0 : lo;
  end = end > G.n_arcs ? G.n_arcs : end;
  int hi = end;
  while (lo < hi) {                                                        // the first arc with sym >= c
    const int mid = (lo + hi) >> 1;
    if (G.sym[mid] < c) lo = mid + 1; else hi = mid;
  }
  return lo < end && G.sym[lo] == c ? lo : -1;
}

// lam(c | the context of node n); arc: the arc it ended on
__device__ __forceinline__ float ngram_walk(const ngram_view& G, int n, int c, int& arc) {
  float acc = 0.f;
  for (int d = 1; d < AVSR_CTC_PREFIX_NGRAM_MAX_ORDER && n != 0; ++d) {
    const int a = ngram_find(G, n, c);
    if (a >= 0) { arc = a; return acc + G.logp[a]; }
    acc += G.bow[n];
    n = ngram_node(G, G.backoff[n]);
  }
  arc = c;                                                                 // the root: one arc per class, c < V <= n_arcs
  return acc + G.logp[c];
}

}  // namespace avsr
