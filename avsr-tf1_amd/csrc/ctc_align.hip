// CTC forced alignment (avsr_ctc_align, include/avsr_hip.h; the rule is INTEGRATION.md section 8): the single most probable alignment
// of a given label row to the frames of the CTC head -- per-frame classes, per-label first / last frames, the path's log-probability
// -- in ONE launch (fp32, gfx950).  Not in the reference.
//
// Work split: one workgroup per utterance, as ctc_loss_kernel's alpha sweep.  Thread i owns the blank state 2i and the label state
// 2i + 1 of the 2U + 1 states; a transition needs the label state of thread i - 1, exchanged through LDS with ONE barrier per frame.
//
// Phases (T_b = frames of the utterance, U its labels):
//   1. lz[t] = log sum_c exp z[t][c] over the real V + 1 classes for t < T_b (16 lanes per row), into the workspace: a state needs only
//      z[t][V] - lz[t] and z[t][its label] - lz[t], so no log-probability row is stored.
//   2. Viterbi forward, t = 0 .. T_b - 1: max where the loss has log-sum-exp.  After every frame the states are shifted by their
//      maximum m_t (it rides the exchange's barrier), the shifts summed in fp64: the score does not lose bits as T grows.  The shift
//      is common to all states of a frame, so it moves no comparison.  After the barrier a thread issues everything it reads from LDS
//      at once (the per-wave maxima as four 16-byte reads, the neighbour's state): one LDS round trip per frame.  Backpointers: 1 bit for a blank state (stay / s - 1), 2 for a
//      label state (stay / s - 1 / s - 2), gathered per wave by three ballots and stored by three lanes as 64-bit words
//      [t][wave][3] in the workspace -- one storage path whatever T is.  Ties: the higher source state wins (strict > going down).
//   3. Backtrace from the end state (the last blank wins a tie with the last label), in blocks of CA_BLOCK frames from the end: the
//      workgroup copies the block's backpointer rows to LDS (contiguous, coalesced), thread 0 walks them there, and after a barrier
//      every thread writes path / frame_lp of one frame of the block.  A frame opens a label's run if its state differs from the
//      previous frame's and closes it if it differs from the next one's, so start / end have exactly one writer: no atomics.
// Every output element is written by every launch: rows t >= T_b and labels j >= U get their padding first, an utterance without a
// valid alignment gets padding everywhere, score 0 and status 0.  Two launches on the same inputs are bit-identical.
#include <stdint.h>
#include "wave.h"
#include "avsr_hip.h"

namespace avsr {

#define CA_BLOCK 128                       // frames per backtrace block

__host__ __device__ static inline int ca_waves(int L) { return L / 64 + 1; }                 // waves that hold threads 0 .. L
__host__ __device__ static inline int ca_threads(int L) {
  const int n = ca_waves(L) * 64;
  return n < 256 ? 256 : n;
}
// dynamic LDS: exO [2][NT + 2], red [2][16], fin [4] floats; st [CA_BLOCK + 2], lab [L] ints (padded to 8 bytes); rows [CA_BLOCK][3 nw] 64-bit
__host__ __device__ static inline size_t ca_lds_words32(int NT, int L) { return (size_t)((2 * (NT + 2) + 32 + 4 + CA_BLOCK + 2 + L + 1) & ~1); }
__host__ __device__ static inline size_t ca_lds_bytes(int NT, int L) { return 4 * ca_lds_words32(NT, L) + 8 * (size_t)CA_BLOCK * 3 * (NT / 64); }
// workspace of one utterance: lz [T] floats (padded to 8 bytes), then the backpointer words [T][3 * ca_waves(L)]
__host__ __device__ static inline int64_t ca_ws_utt_bytes(int T, int L) { return 8 * (((int64_t)T + 1) / 2) + 8 * (int64_t)T * 3 * ca_waves(L); }

// blockDim.x = NT = ca_threads(L): a multiple of 64, > L.  Dynamic LDS: ca_lds_bytes(NT, L).
__global__ __launch_bounds__(1024) void ctc_align_kernel(const avsr_ctc_align_args A) {
  extern __shared__ __attribute__((aligned(16))) float ca_smem[];
  const int NT = blockDim.x, i = threadIdx.x, lane = i & 63, wv = i >> 6, nw = NT >> 6;
  const int b = blockIdx.x, T = A.T, L = A.L, V = A.V;
  const long ld = A.ld;
  const int XS = NT + 2;                  // exchange rows: thread i's value at [i + 1], a -inf sentinel at [0]
  float* exO = ca_smem;                   // [2][XS]  label states
  float* red = exO + 2 * XS;              // [2][16]  per-wave maxima
  float* fin = red + 32;                  // [4]
  int* st = reinterpret_cast<int*>(fin + 4);      // [CA_BLOCK + 2]  states of frames t0 - 1 .. t1 of the block being traced back
  int* lab = st + CA_BLOCK + 2;           // [L]
  uint64_t* rows = reinterpret_cast<uint64_t*>(ca_smem + ca_lds_words32(NT, L));    // [CA_BLOCK][3 * nwu]

  int Tb = A.in_len[b];
  Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
  int U = A.target_len[b];
  U = U < 0 ? 0 : (U > L ? L : U);
  const float* const zb = A.z + (long)b * T * ld;
  int32_t* const pathb = A.path + (long)b * T;
  float* const flpb = A.frame_lp + (long)b * T;
  int32_t* const startb = A.start + (long)b * L;
  int32_t* const endb = A.end + (long)b * L;
  char* const wsb = reinterpret_cast<char*>(A.ws) + (long)b * ca_ws_utt_bytes(T, L);
  float* const lz = reinterpret_cast<float*>(wsb);
  const int nwu = U / 64 + 1, rl = 3 * nwu;                             // waves that hold a state; 64-bit words per backpointer row
  uint64_t* const bp = reinterpret_cast<uint64_t*>(wsb + 8 * (((long)T + 1) / 2));

  for (int j = i; j < L; j += NT) lab[j] = A.labels[(long)b * L + j];
  if (i < 2) exO[i * XS] = -INFINITY;
  __syncthreads();
  const bool hasE = i <= U, hasO = i < U;
  const int li = hasO ? lab[i] : 0;
  const bool badi = hasO && (li < 0 || li >= V);
  const bool repi = hasO && i > 0 && li == lab[i - 1];                // label i repeats label i - 1: no skip over the blank between
  bool ok;
  {   // feasibility, avsr_ctc_loss's: T_b >= U + (adjacent equal pairs), T_b >= 1, every label a real class
    int* ired = reinterpret_cast<int*>(red);
    const int nrep = __popcll(__ballot(repi)), nbad = __popcll(__ballot(badi));
    if (lane == 0) { ired[wv] = nrep; ired[16 + wv] = nbad; }
    __syncthreads();
    int reps = 0, bad = 0;
    for (int w = 0; w < nw; ++w) { reps += ired[w]; bad += ired[16 + w]; }
    __syncthreads();                       // (red is reused below)
    ok = Tb >= 1 && !bad && Tb >= U + reps;
  }
  // padding first: frames past T_b, labels past U; everything of an utterance that cannot be aligned
  const int Tv = ok ? Tb : 0, Uv = ok ? U : 0;
  for (int t = Tv + i; t < T; t += NT) { pathb[t] = -1; flpb[t] = 0.f; }
  for (int j = Uv + i; j < L; j += NT) { startb[j] = -1; endb[j] = -1; }
  if (!ok) {
    if (i == 0) { A.score[b] = 0.f; A.status[b] = 0; }
    return;
  }
  if (i < 32) red[i] = -INFINITY;          // all 16 slots of both halves: the sweep reads a half whole (ordered by phase 1's barrier)

  // ---- phase 1: the rows' normalisers -------------------------------------------------------------------------------------------
  {
    const int g = i >> 4, j = i & 15, ng = NT >> 4, C = V + 1;
    for (int t0 = 0; t0 < Tb; t0 += ng) {
      const int t = t0 + g;
      const bool on = t < Tb;
      const float* zr = zb + (long)(on ? t : 0) * ld;
      float mx = -INFINITY;
      for (int c = j; c < C; c += 16) mx = fmaxf(mx, zr[c]);
      mx = group16_max(mx);
      float s = 0.f;
      for (int c = j; c < C; c += 16) s += expf(zr[c] - mx);
      s = group16_sum(s);
      if (on && j == 0) lz[t] = mx + logf(s);
    }
  }
  __syncthreads();                         // lz is visible to the whole workgroup

  // ---- phase 2: Viterbi forward -------------------------------------------------------------------------------------------------
  float e, o;                              // shifted scores of states 2i / 2i + 1
  double msum = 0.0;
  {
    {
      const float n0 = lz[0];
      e = i == 0 ? zb[V] - n0 : -INFINITY;
      o = (i == 0 && hasO) ? zb[li] - n0 : -INFINITY;
    }
    // The blank's logit, the label's and the normaliser of the frame after next, fetched off the chain.  Unconditional, from a clamped
    // row (past the end: the last frame again, never used), and subtracted only where they are used: a load under a branch, or one
    // whose result is combined at once, is waited for right there, which puts the memory latency on the chain.
    const int t1 = Tb > 1 ? 1 : 0;
    float nB = zb[(long)t1 * ld + V], nL = zb[(long)t1 * ld + li], nN = lz[t1];
    for (int t = 0; t < Tb; ++t) {
      const bool more = t + 1 < Tb;
      const float cB = nB, cL = nL, cN = nN;                             // frame t + 1
      {
        const int tn = t + 2 < Tb ? t + 2 : Tb - 1;
        nB = zb[(long)tn * ld + V]; nL = zb[(long)tn * ld + li]; nN = lz[tn];
      }
      const int buf = t & 1;
      const float mx = wave64_max(fmaxf(e, o));
      exO[buf * XS + i + 1] = o;
      if (lane == 0) red[buf * 16 + wv] = mx;
      lds_barrier();
      // one LDS round trip for everything the step reads: the 16 slots of the half (waves that do not exist left -inf there) as
      // four 16-byte reads, and the neighbour's label state
      const float4* r4 = reinterpret_cast<const float4*>(red + buf * 16);
      const float4 q0 = r4[0], q1 = r4[1], q2 = r4[2], q3 = r4[3];
      const float ox = exO[buf * XS + i];
      float m = fmaxf(fmaxf(fmaxf(fmaxf(q0.x, q0.y), fmaxf(q0.z, q0.w)), fmaxf(fmaxf(q1.x, q1.y), fmaxf(q1.z, q1.w))),
                      fmaxf(fmaxf(fmaxf(q2.x, q2.y), fmaxf(q2.z, q2.w)), fmaxf(fmaxf(q3.x, q3.y), fmaxf(q3.z, q3.w))));
      if (m == -INFINITY) m = 0.f;
      e -= m; o -= m;
      msum += (double)m;
      if (more) {
        const float yB = cB - cN, yL = cL - cN;
        const float om1 = ox - m;                                        // label i - 1 (state 2i - 1); -inf for thread 0
        // ties go to the higher source state: stay, then s - 1, then s - 2
        const bool kE = om1 > e;
        int kO = 0;
        float bo = o;
        if (e > bo) { bo = e; kO = 1; }
        if (!repi && om1 > bo) { bo = om1; kO = 2; }
        const float ne = hasE ? yB + (kE ? om1 : e) : -INFINITY;
        const float no = hasO ? yL + bo : -INFINITY;
        e = ne; o = no;
        const uint64_t w0 = __ballot(kE), w1 = __ballot(kO & 1), w2 = __ballot(kO >> 1);
        if (wv < nwu && lane < 3) bp[(long)(t + 1) * rl + wv * 3 + lane] = lane == 0 ? w0 : (lane == 1 ? w1 : w2);
      }
    }
  }
  // (the loop leaves e, o = the shifted scores of frame T_b - 1: its last pass computes no successor)
  if (i == U) { fin[0] = e; if (U == 0) fin[1] = -INFINITY; }
  if (U > 0 && i == U - 1) fin[1] = o;
  __syncthreads();                         // fin; and every backpointer word is visible to the whole workgroup
  const bool endLabel = fin[1] > fin[0];   // the last blank wins a tie
  const float best = endLabel ? fin[1] : fin[0];
  if (!(best > -INFINITY && best < INFINITY)) {            // (not reachable with finite logits: the alignment exists)
    for (int t = i; t < Tb; t += NT) { pathb[t] = -1; flpb[t] = 0.f; }
    for (int j = i; j < U; j += NT) { startb[j] = -1; endb[j] = -1; }
    if (i == 0) { A.score[b] = 0.f; A.status[b] = 0; }
    return;
  }
  if (i == 0) { A.score[b] = (float)(msum + (double)best); A.status[b] = 1; }

  // ---- phase 3: backtrace in blocks of frames, from the end ----------------------------------------------------------------------
  int s = endLabel ? 2 * U - 1 : 2 * U;    // thread 0: state of frame t1 - 1 of the block
  int snext = -1;                          // thread 0: state of frame t1 (-1: there is none)
  for (int t1 = Tb; t1 > 0; t1 -= CA_BLOCK) {
    const int t0 = t1 > CA_BLOCK ? t1 - CA_BLOCK : 0, n = t1 - t0;
    {   // rows t0 .. t1 - 1 of the backpointers (row 0 does not exist: nothing leads into frame 0)
      const int r0 = t0 > 0 ? t0 : 1;
      const long g0 = (long)r0 * rl;
      const int cnt = (t1 - r0) * rl, off = (r0 - t0) * rl;
      for (int k = i; k < cnt; k += NT) rows[off + k] = bp[g0 + k];
    }
    __syncthreads();
    if (i == 0) {
      st[n + 1] = snext;
      for (int t = t1 - 1; t >= t0; --t) {
        st[t - t0 + 1] = s;
        if (t > 0) {
          const int idx = s >> 1;
          const uint64_t* r = rows + (t - t0) * rl + (idx >> 6) * 3;
          const uint64_t w0 = r[0], w1 = r[1], w2 = r[2];
          const int sh = idx & 63;
          const int kE = (int)((w0 >> sh) & 1), kO = (int)((w1 >> sh) & 1) | ((int)((w2 >> sh) & 1) << 1);
          s -= (s & 1) ? kO : kE;
          s = s < 0 ? 0 : s;                // (a finite state's backpointer never leads below state 0: this guards the LDS index only)
        }
      }
      st[0] = t0 > 0 ? s : -1;             // state of frame t0 - 1: where the next block starts
      snext = st[1];
    }
    __syncthreads();
    for (int k = i; k < n; k += NT) {
      const int t = t0 + k, sc = st[k + 1], sp = st[k], sn = st[k + 2];
      const int j = sc >> 1;
      const int cls = (sc & 1) ? lab[j] : V;
      pathb[t] = cls;
      flpb[t] = zb[(long)t * ld + cls] - lz[t];
      if (sc & 1) {
        if (sp != sc) startb[j] = t;
        if (sn != sc) endb[j] = t;
      }
    }
    // (no barrier here: the next block's copy writes rows only, and its barrier comes before thread 0 writes st again)
  }
}

}  // namespace avsr

using namespace avsr;

extern "C" int avsr_ctc_align_supported(int32_t V, int32_t L) {
  return (V >= 1 && L >= 1 && L <= AVSR_CTC_ALIGN_MAX_L) ? 1 : 0;
}

extern "C" int64_t avsr_ctc_align_ws_bytes(int32_t B, int32_t T, int32_t L) {
  if (B <= 0 || T <= 0 || L <= 0) return 0;
  return (int64_t)B * ca_ws_utt_bytes(T, L);
}

extern "C" int avsr_ctc_align(const avsr_ctc_align_args* a, void* stream) {
  if (!a || !a->z || !a->labels || !a->target_len || !a->in_len || !a->score || !a->status || !a->path || !a->frame_lp || !a->start ||
      !a->end || !a->ws)
    return AVSR_ERR_ARG;
  if (a->B <= 0 || a->T <= 0 || a->L <= 0 || a->V <= 0 || a->ld < (int64_t)a->V + 1) return AVSR_ERR_ARG;
  if (((uintptr_t)a->ws & 7) != 0) return AVSR_ERR_ARG;                 // the backpointer words are 64-bit
  if (!avsr_ctc_align_supported(a->V, a->L)) return AVSR_ERR_UNSUPPORTED;
  if (a->ws_bytes < avsr_ctc_align_ws_bytes(a->B, a->T, a->L)) return AVSR_ERR_ARG;
  const int NT = ca_threads(a->L);
  hipLaunchKernelGGL(ctc_align_kernel, dim3(a->B), dim3(NT), ca_lds_bytes(NT, a->L), (hipStream_t)stream, *a);
  AVSR_CHECK_LAUNCH();
  return AVSR_OK;
}
