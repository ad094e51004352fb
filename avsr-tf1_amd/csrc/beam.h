// The beam-search selection step (csrc/beam.hip) and the per-step terms queued ahead of it (beam_lm.hip, beam_ngram.hip, beam_word_ngram.hip, beam_ctc.hip): what the
// decoder's scheduler (attn_rnn.hip) and the C entries call.
#pragma once
#include "common.h"
#include "avsr_hip.h"

namespace avsr {

// One selection step over n_utt utterances of K beams (R = n_utt * K hypothesis rows): the arguments of beam_step_kernel, host side.
struct BeamStep {
  float* logits; long logits_sb;                    // this step's [R][V], rows logits_sb apart: given, or written when the output layer runs inside
  int n_utt, K, V, step, eos;
  float length_penalty;                             // GNMT length-penalty weight
  const float* logp_in; const int32_t* fin_in; const int32_t* len_in;      // beam state [R] the step reads ...
  float* logp_out; int32_t* fin_out; int32_t* len_out;                     // ... and writes
  int32_t* tok; int32_t* parent_rows;               // [R] symbol and parent row of every new hypothesis
  int32_t* step_ids; int32_t* parent_ids;           // records [steps][R]: row `step` is written
  int32_t* n_unfinished;                            // [steps] counters (zeroed by the caller): [step] is added to, [step - 1] is read
  const float* x; long x_sb; int O;                 // output layer inside the step: its input rows [R][O], x_sb apart ...
  const float* wout_t; const float* bout;           // ... Wout^T [V][O] and the bias [V]
  const float* extra; float extra_weight;           // additive term [R][V] of the unfinished beams (LM / CTC), NULL: none
};

inline bool beam_step_fits(long K, long V) { return K * V <= 1024; }   // the kernel keeps a thread's candidates in registers (4 x 256)

// 16-column tiles of the output layer where it can run inside the step, 0 where it cannot (the caller then computes the logits ahead of it)
inline int beam_step_nct(const BeamStep& s) {
  if (s.K > 16 || s.V > 64 || s.O % 256 != 0 || s.x_sb % 4 != 0 || (((uintptr_t)s.x | (uintptr_t)s.wout_t) & 15) != 0) return 0;
  return s.V <= 32 ? 2 : 4;
}

// The only launch site of beam_step_kernel.  allow_inside && s.x: the output layer runs inside the step (AVSR_ERR_UNSUPPORTED where
// beam_step_nct says it cannot); otherwise s.logits holds the logits and x is ignored.
int beam_step_launch(const BeamStep& s, bool allow_inside, hipStream_t stream);

int beam_lm_check(const avsr_beam_lm* m);                                           // beam_lm.hip: the language-model step
int beam_lm_step_launch(const avsr_beam_lm& m, const int32_t* tok, const int32_t* parent_rows, int step, hipStream_t s);
int beam_ngram_check(const avsr_beam_ngram* g);                                     // beam_ngram.hip: the back-off n-gram step
int beam_ngram_step_launch(const avsr_beam_ngram& g, const int32_t* tok, const int32_t* parent_rows, int step, hipStream_t s);
int beam_word_ngram_check(const avsr_beam_word_ngram* g);                           // beam_word_ngram.hip: the word-level n-gram step
int beam_word_ngram_step_launch(const avsr_beam_word_ngram& g, const int32_t* tok, const int32_t* parent_rows, int step, hipStream_t s);
int beam_ctc_check(const avsr_beam_ctc* c);                                         // beam_ctc.hip: the CTC prefix-score step
int beam_ctc_begin_launch(const avsr_beam_ctc& c, hipStream_t s);
int beam_ctc_step_launch(const avsr_beam_ctc& c, const int32_t* tok, const int32_t* parent_rows, const int32_t* fin, int step, hipStream_t s);
int beam_ctc_combine_launch(const float* term, float weight, const float* lm_logp, float lm_weight, float* extra, long n, hipStream_t s);

}  // namespace avsr
