"""fp64 reference of attention rescoring (csrc/rescore.hip): the log-probability of a teacher-forced label row,
the combination with the CTC score and the stable selection; the inputs the GPU kernel test uses; a float32 restatement of the score
that sizes the tolerance; and the oracle's evaluation-mode teacher-forced decoder on given label rows.

TOL_SCORE is computed HERE, at import, and printed: 8 x the largest deviation of the float32 restatement (row-wise max-subtracted
log-softmax in float32, the rows added in float32 in ascending t) from fp64 over kernel_cases() -- the very inputs
tests/test_gpu_rescore.py launches.  Nothing about it comes from the kernel."""
import itertools

import numpy as np
import torch

NEG = -np.inf
KERNEL_V, KERNEL_L, KERNEL_B = (2, 15, 31, 41, 257), (1, 7, 40), (1, 3, 64)
PEAK = 80.0                                                 # tests/regime.py's peaked regime: logits of magnitude 80


def seq_logprob(logits, labels, lens):
    """out[b] = sum_{t < min(lens[b], L)} log_softmax(logits[b, t])[labels[b, t]] in fp64; lens[b] <= 0 gives 0.0; a label outside
    0 .. V-1 contributes -inf."""
    z = torch.from_numpy(np.array(logits, dtype=np.float64))
    B, L, V = z.shape
    y = torch.log_softmax(z, dim=-1).numpy()
    labels, lens = np.asarray(labels), np.asarray(lens)
    out = np.zeros(B, np.float64)
    for b in range(B):
        for t in range(int(np.clip(lens[b], 0, L))):
            v = int(labels[b, t])
            out[b] += y[b, t, v] if 0 <= v < V else NEG
    return out


def seq_logprob_f32(logits, labels, lens):
    """The same in float32 throughout, as a plain fp32 implementation would do it: what float32 itself loses on these inputs."""
    z = np.asarray(logits, np.float32)
    B, L, V = z.shape
    labels, lens = np.asarray(labels), np.asarray(lens)
    out = np.zeros(B, np.float32)
    for b in range(B):
        acc = np.float32(0.0)
        for t in range(int(np.clip(lens[b], 0, L))):
            row = z[b, t]
            m = row.max()
            s = np.exp(row - m, dtype=np.float32).sum(dtype=np.float32)
            v = int(labels[b, t])
            lp = np.float32(np.float32(row[v] - m) - np.log(s, dtype=np.float32)) if 0 <= v < V else np.float32(NEG)
            acc = np.float32(acc + lp)
        out[b] = acc
    return out


def select(s_att, s_ctc, n, weight):
    """(order [B, K] int, final [B, K]): final[k] = s_att[k] + weight * s_ctc[k] (weight == 0: s_att[k], no product) over k < n[b], sorted
    by final descending, ties to the lower k; slots >= n[b]: order -1, final -inf.  Computed in the dtype of s_att (float32 inputs
    of small dyadic rationals give exact float32 results; float64 inputs give the fp64 reference)."""
    s_att, s_ctc = np.asarray(s_att), np.asarray(s_ctc)
    dt = s_att.dtype
    B, K = s_att.shape
    order, final = np.full((B, K), -1, np.int32), np.full((B, K), NEG, dt)
    for b in range(B):
        nb = int(np.clip(n[b], 0, K))
        f = s_att[b, :nb].copy() if weight == 0 else (s_att[b, :nb] + dt.type(weight) * s_ctc[b, :nb].astype(dt)).astype(dt)
        ks = sorted(range(nb), key=lambda k: (-f[k], k))
        order[b, :nb], final[b, :nb] = ks, f[ks]
    return order, final


def lens_for(B, L, rng):
    """Mixed label lengths: 0, a value above L, the full length, the rest drawn from 1 .. L."""
    lens = rng.integers(1, L + 1, B).astype(np.int32)
    lens[0] = L
    if B >= 3:
        lens[1], lens[2] = 0, L + 2
    return lens


def kernel_case(V, L, B, peaked=False):
    """(logits [B, L, V] float32, labels [B, L] int32, lens [B] int32), a function of the shape alone; read-only."""
    rng = np.random.default_rng(1000 * V + 10 * L + B + (7 if peaked else 0))
    labels = rng.integers(0, V, (B, L)).astype(np.int32)
    if peaked:                                              # one logit at +80, the others at -80; the label on the peak or off it
        z = np.full((B, L, V), -PEAK, np.float32)
        peak = rng.integers(0, V, (B, L))
        np.put_along_axis(z, peak[..., None], PEAK, axis=-1)
        on = rng.random((B, L)) < 0.7
        labels = np.where(on, peak, labels).astype(np.int32)
    else:
        z = (rng.standard_normal((B, L, V)) * 3.0).astype(np.float32)
    lens = lens_for(B, L, rng)
    for a in (z, labels, lens):
        a.setflags(write=False)
    return z, labels, lens


def kernel_cases():
    """Every input of the GPU kernel test: the shape grid, plus the peaked family at every V."""
    for V, L, B in itertools.product(KERNEL_V, KERNEL_L, KERNEL_B):
        yield (V, L, B, False), kernel_case(V, L, B)
    for V in KERNEL_V:
        yield (V, 7, 3, True), kernel_case(V, 7, 3, peaked=True)


_REF = {}


def kernel_reference(V, L, B, peaked=False):
    """fp64 scores of a kernel case, computed once."""
    return _REF[(V, L, B, peaked)]


def _measure():
    worst = 0.0
    for key, (z, labels, lens) in kernel_cases():
        ref = seq_logprob(z, labels, lens)
        _REF[key] = ref
        f32 = seq_logprob_f32(z, labels, lens).astype(np.float64)
        assert np.isfinite(ref).all() and np.isfinite(f32).all()
        worst = max(worst, float(np.abs(f32 - ref).max()))
    return worst


F32_DEVIATION = _measure()
TOL_SCORE = 8 * F32_DEVIATION
print("ref_rescore: float32 restatement deviates from fp64 by at most %.3g on the kernel inputs; TOL_SCORE = %.3g" % (F32_DEVIATION, TOL_SCORE))


# ------------------------------------------------------------------------------------------------
# the oracle's decoder, evaluation mode, teacher-forced on given label rows
def oracle_eval_model(O, W, ocfg, batch):
    """(P, m): the oracle's model on `batch` with encoders and batch norms in evaluation mode (training=False: moving statistics, no
    dropout); the CTC head's variables are not the oracle's."""
    P = O.to_torch({k: v for k, v in W.items() if "/ctc/" not in k})
    with torch.no_grad():
        return P, O._Model(P, ocfg, batch, False, torch.float64)


def teacher_forced_logits(O, P, m, ocfg, labels, labels_len):
    """The loop of oracle.forward_train on the label rows `labels` [B, L] (fed GO-prefixed) without dropout and without sampling:
    logits [B, L, V] fp64, zeros at steps t >= labels_len[b] (TrainingHelper's impute_finished)."""
    labels = torch.as_tensor(np.asarray(labels), dtype=torch.int64)
    ll = torch.as_tensor(np.asarray(labels_len), dtype=torch.int64)
    B, L = labels.shape
    V = ocfg.vocab_size
    fed = torch.cat([torch.full((B, 1), ocfg.go_id, dtype=torch.int64), labels], dim=1)[:, :L]
    out = np.zeros((B, L, V), np.float64)
    with torch.no_grad():
        state, att = m.init_state, torch.zeros(B, m.att_dim, dtype=torch.float64)
        for t in range(int(ll.max()) if B else 0):
            o, ns, natt, _ = m.step(O._embedding(P, ocfg)[fed[:, t]], state, att, t)
            lg = m.logits(o)
            fin = (t >= ll)[:, None]
            out[:, t] = torch.where(fin, torch.zeros_like(lg), lg).numpy()
            state = O._map_state(lambda n, s: torch.where(fin, s, n), ns, state)
            att = torch.where(fin, att, natt)
    return out
