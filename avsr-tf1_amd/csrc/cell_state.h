// The rolling state of one recurrent cell across the per-step launches: the `state` / `dstate` scratch of avsr_rnn_layer,
// avsr_dec_layer and avsr_attn_rnn (include/avsr_hip.h).  This file is the layout's one description; the fused decoder
// kernels (dec_persist*.hip) take its slot constants, everything on the host its accessors.
//
// Both buffers are rows of SLOTS of B*H floats (B rows, H = the layer's units); a [2] pair ping-pongs on the parity of the step.
//   state   h[2] | c[2] | x~[2]                                 4*B*H floats; 6*B*H with dropout or a residual layer
//           h, c: the recurrent state.  A GRU has no c: the first c slot holds r*h of the running step.
//           x~:   the layer's EMITTED output as its consumer sees it (output mask x consumer's input mask, or h + input)
//   dstate  LSTM  dG[2][B][4H] | dc[2] | dh_carry[2] | dres[2]   12*B*H floats; 14*B*H for a residual layer
//           GRU   dGg[2][B][2H] | dpc[2] | carry[2] | tmp[2] | (2 unused) | dres[2]
//           dG / dGg: d(gate pre-activations), dpc: d(candidate pre-activation), dc / dh_carry / carry: the gradient handed to step
//           t-1, tmp: du and dh*u between the two GRU phases, dres: d(emitted output) a residual layer hands to the layer below.
#pragma once

namespace avsr {

enum { ST_H = 0, ST_C = 2, ST_RH = 2, ST_X = 4,                      // slots of `state`
       DS_DG = 0, DS_DC = 8, DS_DH = 10, DS_DRES = 12,              // slots of an LSTM's `dstate` (dG: 4 slots per parity)
       DG_DGG = 0, DG_DPC = 4, DG_CARRY = 6, DG_TMP = 8 };          // slots of a GRU's `dstate` (dGg: 2 slots per parity)

static inline float* cell_slot(float* base, int B, int H, int slot) { return base + (long)slot * B * H; }
static inline float* st_h(float* s, int B, int H, int p) { return cell_slot(s, B, H, ST_H + p); }
static inline float* st_c(float* s, int B, int H, int p) { return cell_slot(s, B, H, ST_C + p); }
static inline float* st_rh(float* s, int B, int H) { return cell_slot(s, B, H, ST_RH); }
static inline float* st_x(float* s, int B, int H, int p) { return cell_slot(s, B, H, ST_X + p); }
static inline float* ds_dg(float* ds, int B, int H, int p) { return cell_slot(ds, B, H, DS_DG + 4 * p); }
static inline float* ds_dc(float* ds, int B, int H, int p) { return cell_slot(ds, B, H, DS_DC + p); }
static inline float* ds_dh(float* ds, int B, int H, int p) { return cell_slot(ds, B, H, DS_DH + p); }
static inline float* ds_dres(float* ds, int B, int H, int p) { return cell_slot(ds, B, H, DS_DRES + p); }
static inline float* dg_dgg(float* ds, int B, int H, int p) { return cell_slot(ds, B, H, DG_DGG + 2 * p); }
static inline float* dg_dpc(float* ds, int B, int H, int p) { return cell_slot(ds, B, H, DG_DPC + p); }
static inline float* dg_carry(float* ds, int B, int H, int p) { return cell_slot(ds, B, H, DG_CARRY + p); }
static inline float* dg_tmp(float* ds, int B, int H, int which) { return cell_slot(ds, B, H, DG_TMP + which); }

}  // namespace avsr
