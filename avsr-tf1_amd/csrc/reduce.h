// Entry points of the column reductions (reduce.hip) that other translation units call.
#pragma once
#include "common.h"

namespace avsr {
// The final reduction of a set of partial slabs (a FinalJob of reduce.hip): out[f] = alpha * sum_i part[i * ld + column(f)] + beta * out[f].
// kind 0: columns [0, split) -> out, [split, F) -> out2 (split >= F: no out2);  kind 1: the pixel-pair slab of an 8-channel weight gradient
// (conv_wgrad.hip; F is not read).  Between avsr_slab_defer_begin and _end the job is only recorded -- the slabs must stay untouched
// until _end, which runs every recorded job in one launch -- otherwise it is launched here.  Either way the same kernel sums in the same order.
int slab_reduce(const float* part, long ld, int nblk, int F, float* out, float* out2, int split, int kind, int Ci, float alpha, float beta,
                hipStream_t s);
bool slab_deferring();
}  // namespace avsr

// The final pass alone, over nblk partial rows written by another kernel: out[f] = alpha * sum_i part[i][f] + beta * out[f].
// _split: rows `ld` floats apart (F <= ld), columns [0, split) -> out, [split, F) -> out2.
int avsr_colsum_final_launch(const float* part, int nblk, float* out, int F, float alpha, float beta, void* stream);
int avsr_colsum_final_launch_split(const float* part, long ld, int nblk, float* out, float* out2, int split, int F, float alpha, float beta,
                                   void* stream);
