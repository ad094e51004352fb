// Launch descriptor of beam_gemm_kernel (csrc/beam_gemm.hip): 64 x 64-tiled products over hypothesis rows whose operand rows are gathered
// while they are staged.  Shared by the decoder's beam-search steps (beam_gemm.hip) and the language-model step (beam_lm.hip).
#pragma once
#include "common.h"
#include "avsr_hip.h"

namespace avsr {

#define BG_MAX_SRC 3
#define BG_MAX_PROB 2
#define BG_T 64            // tile rows = tile columns
#define BG_K 128           // K per stage

struct BGSrc { const float* a; long sb; const int* gather; int K, pad; };
struct BGProb {
  BGSrc src[BG_MAX_SRC];
  int nsrc, R, N, tile0, ntx, pad;
  const float* wt; long ldw;                     // weights [N][ldw], K contiguous
  float* out; long out_sb;                       // LINEAR: out[r * out_sb + n]
  const float* bias; const float* c_in; const int* parent; float* c_out; float* h_out; float* seq_out; long seq_sb;   // LSTM
};
struct BGLaunch { int nprob, ntiles; BGProb p[BG_MAX_PROB]; };

// launches beam_gemm_kernel<lstm> over G.ntiles workgroups
int beam_gemm_launch(const BGLaunch& G, bool lstm, hipStream_t s);

// The decoder's beam-search steps on the tiled kernel (mode 3 of avsr_attn_rnn_fwd).  g_beam_dense is avsr_attn_rnn_set_beam_kernel's
// switch; the two launches return AVSR_ERR_UNSUPPORTED where the tiled kernel does not apply (the caller then runs step_kernel).
extern int g_beam_dense;
bool beam_dense_on();
int beam_cell_launch(const avsr_attn_rnn& d, int l, hipStream_t s);
int beam_attention_layer_launch(const avsr_attn_rnn& d, int l, hipStream_t s);

}  // namespace avsr
