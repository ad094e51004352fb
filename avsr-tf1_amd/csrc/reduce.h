// Entry points of the column reductions (reduce.hip) that other translation units call.
#pragma once
#include "common.h"

namespace avsr {
// Record the final reduction of a set of partial slabs instead of launching it (between avsr_slab_defer_begin and _end);
// false: not deferring, the caller launches as before.  kind 0: columns [0, split) -> out, [split, F) -> out2;
// kind 1: the pixel-pair slab of an 8-channel weight gradient (conv_wgrad.hip), alpha is not applied.
bool slab_defer_push(const float* part, long ld, int nblk, int F, float* out, float* out2, int split, int kind, int Ci, float alpha, float beta,
                     hipStream_t s);
bool slab_deferring();
}  // namespace avsr

// The final pass alone, over nblk partial rows written by another kernel: out[f] = alpha * sum_i part[i][f] + beta * out[f].
// _ld: rows `ld` floats apart (F <= ld);  _split: columns [0, split) -> out, [split, F) -> out2.
int avsr_colsum_final_launch(const float* part, int nblk, float* out, int F, float alpha, float beta, void* stream);
int avsr_colsum_final_launch_ld(const float* part, long ld, int nblk, float* out, int F, float alpha, float beta, void* stream);
int avsr_colsum_final_launch_split(const float* part, long ld, int nblk, float* out, float* out2, int split, int F, float alpha, float beta,
                                   void* stream);
