"""Reference, case table and checker of the attention-decoder conformance suite (tests/test_dec_check_cpu.py judges them on the CPU,
tests/test_gpu_dec_conformance.py runs avsr_attn_rnn_fwd / avsr_attn_rnn_bwd against them).  A plain helper module, not a conftest.

The reference restates include/avsr_hip.h ("Attention-wrapped LSTM over a sequence") and the per-step scheduler (csrc/attn_rnn.hip, the
definition of the block) as an explicit step loop in torch at a given dtype:
  * step l of row b is live while l < steplen[b]; a dead step carries the state through and emits zeros (cell_out, att, attd, hs_seq,
    logits); the LSTM has forget bias 1 and cell clip +-1, gate order i, j, f, o, gate columns unit-interleaved (4*unit + gate);
  * the cell input is [x_l | attention_{l-1} | h_{l-1}] against the rows [E | A | H] of the kernel; mode 0 finds x.Wx in `gates` (an INPUT:
    fp64 product rounded once to fp32, so no GEMM is part of the suite), mode 2 reads xs[b][l], mode 1 the embedding of tok[b];
  * per memory: raw score (Luong: keys . q, recorded un-scaled; Bahdanau: v . tanh(keys + q.Wq (+ b))), softmax over t < len of the scaled
    score, context over the values, attention = [cell_out | ctx] . W_att; the records hold the raw scores at t < len, the context, the
    processed query and the softmax statistics (max, exp-sum: compared merged over whatever chunks a form records);
  * DropoutWrapper masks are oracle.hash_u32 / uniform01 bits: stream cell_id*4 + {0 in, 1 state, 2 out}; the output / state index is
    (b*L + l)*H + unit, the input index (b*L + l)*(E + A) + column with the attention of step l consumed at time l + 1;
  * mode 2 draws select (stream 1000) and the categorical sample (stream 1001, oracle.categorical_f32 on the fp32 logits) at index b*L + l
    for EVERY row and every l + 1 < L, and writes fed[b][l+1] and the (input-dropped) embedding row xs[b][l+1];
  * mode 1 takes the first maximum, writes ids (0 once finished), tok, and sets steplen when EOS is emitted;
  * the backward is autograd of a random linear probe on the emitted attention, the emitted cell output (both zero at dead steps, as a
    loss makes them) and the final states; it is read off at dgates (d pre-activation), datt, dh0, dc0 and per memory dscores (d of the
    SCALED score), dctx, dpq.  No GEMM, memory layer or deferred gradient is part of the suite.
The same function at torch.float32 is the fp32 twin whose distance from the fp64 run is the `noise` of a case."""
import dataclasses
from typing import Optional, Tuple

import numpy as np
import torch

from oracle.avsr_oracle import categorical_f32, uniform01
import ref_rnn

T_SUITE = 2e-5              # forward records, states, logits: the recurrent suite's figure for records (ref_rnn.T_SUITE)
T_SUITE_BPTT = 2e-4         # x max(1, max|ref|) on the BPTT outputs (ref_rnn.T_SUITE_DGATES)
NOISE_CAP = ref_rnn.NOISE_CAP
GUARD = ref_rnn.GUARD
PATTERN = ref_rnn.PATTERN
MARGIN_FACTOR = 100         # an argmax must lead, and a sampling uniform keep from the edges of its CDF bin, by this x the case's logits bound
TYPES = ("luong", "scaled_luong", "bahdanau", "normed_bahdanau")
GO, EOS = 1, 2
CELL_ID = 40
FUSED_SETTINGS = (0, 1, 2, 3)          # avsr_attn_rnn_set_fused: per-step, fused both, forward only, backward only


# ---- the case table -------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Mem:
    type: str
    T: int
    D: int

    @property
    def chunk(self):                    # the per-step kernels' chunk, chosen as the model chooses it
        return 64 if self.T > 64 else max(16, (self.T + 1) // 2)

    @property
    def nchunk(self):
        return (self.T + self.chunk - 1) // self.chunk


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    modes: Tuple[int, ...]
    mems: Tuple[Mem, ...]
    B: int
    L: int
    H: int
    E: int
    Vs: Tuple[int, ...] = (28,)
    plan: dict = None                   # mode -> None (declined: per-step) | dict(variant=, rows=, quarter=, launches=[, lds_fwd=, lds_bwd=])
    drop: Optional[Tuple[float, float, float]] = None      # keep_in, keep_state, keep_out
    prob: float = 0.0                   # sampling_prob (mode 2)
    h0: bool = True                     # h0 / c0 given (False: NULL)
    finals: bool = True                 # dh_final / dc_final given (False: NULL)
    prof_tag: int = 0
    seed: int = 0
    split: bool = False                 # modes 1 and 2: also issue the forward as [0, 2) then [2, L)

    @property
    def oa(self):
        return int(self.mems[0].type in ("luong", "scaled_luong"))

    def keys(self):
        """The (mode, V) pairs this row runs at (V = 0 in mode 0: no output layer)."""
        return [(m, V) for m in self.modes for V in ((0,) if m == 0 else self.Vs)]


def _p(variant, quarter, rows=8, launches=1, **kw):
    return dict(variant=variant, rows=rows, quarter=tuple(quarter), launches=launches, **kw)


def _table():
    Lu, SL = "luong", "scaled_luong"
    C = [
        Case("min_empty_quarter", (2,), (Mem(Lu, 5, 16),), 3, 4, 16, 16, plan={2: _p(0, (2,))}, seed=11),
        Case("T1_L1_B1", (1, 2), (Mem(Lu, 1, 16),), 1, 1, 16, 16, plan={1: _p(0, (1,)), 2: _p(0, (1,))}, seed=20),
        Case("scaled_D_ne_H_drop", (2,), (Mem(SL, 37, 80),), 11, 5, 48, 32, Vs=(32,), plan={2: _p(0, (10,))}, drop=(0.8, 0.9, 0.7),
             prob=0.3, seed=30, split=True),
        Case("v33", (1, 2), (Mem(SL, 37, 80),), 11, 5, 48, 32, Vs=(33,), plan={1: _p(0, (10,)), 2: _p(0, (10,))}, drop=(0.8, 0.9, 0.7),
             prob=0.3, seed=40),
        Case("two_q32", (1, 2), (Mem(Lu, 128, 16), Mem(SL, 129, 32)), 9, 4, 32, 16, plan={1: _p(1, (32, 33)), 2: _p(1, (32, 33))}, seed=50),
        Case("two_v2", (0, 1, 2), (Mem(Lu, 129, 32), Mem(SL, 9, 16)), 9, 4, 32, 16, Vs=(28, 41),
             plan={m: _p(2, (33, 3)) for m in (0, 1, 2)}, prob=0.3, seed=60, split=True),
        Case("two_mode0_v1", (0,), (Mem(Lu, 9, 16), Mem(Lu, 129, 32)), 9, 4, 32, 48, plan={0: _p(1, (3, 33))}, seed=70),
        Case("two_both_wide", (2,), (Mem(Lu, 129, 16), Mem(Lu, 129, 32)), 9, 3, 32, 16, plan={2: None}, seed=80),
        Case("q128", (2,), (Mem(Lu, 512, 16),), 2, 2, 16, 16, plan={2: _p(0, (128,))}, seed=90),
        Case("q129", (2,), (Mem(Lu, 513, 16),), 2, 2, 16, 16, plan={2: None}, seed=100),
        Case("attentive_r16", (0,), (Mem(Lu, 128, 32),), 19, 5, 32, 48, plan={0: _p(3, (64,), rows=16)}, drop=(0.8, 0.9, 0.7), prof_tag=1,
             seed=110),
        Case("attentive_129", (0,), (Mem(Lu, 129, 32),), 19, 5, 32, 48, plan={0: _p(0, (33,))}, seed=120),
        Case("attentive_b131", (0,), (Mem(Lu, 9, 16),), 131, 3, 16, 16, plan={0: _p(3, (5,), rows=16, launches=2)}, seed=130),
        Case("dec_b67", (2,), (Mem(Lu, 6, 16), Mem(Lu, 3, 16)), 67, 3, 16, 16, plan={2: _p(1, (2, 1), launches=2)}, prob=0.3, seed=140),
        Case("bahdanau", (1, 2), (Mem("bahdanau", 41, 48),), 9, 5, 32, 16, Vs=(28, 41), plan={1: _p(4, (11,)), 2: _p(4, (11,))}, prob=0.3,
             seed=150, split=True),
        Case("normed_bahdanau", (1, 2), (Mem("normed_bahdanau", 41, 48),), 9, 5, 32, 16, Vs=(28, 41), plan={1: _p(4, (11,)), 2: _p(4, (11,))},
             prob=0.3, seed=160),
        Case("bahdanau_mode0", (0,), (Mem("bahdanau", 41, 48),), 9, 4, 32, 16, plan={0: None}, seed=170),
        # NC = 8 + 32 + 16 = 56 sixteen-wide chunks of the cell product: ceil(56 / 8) = 7 = DP_CPW per wave; UW = 8, AW = 16
        Case("wide_cpw7", (2,), (Mem(Lu, 19, 256), Mem(Lu, 60, 256)), 9, 3, 256, 128, plan={2: _p(1, (5, 15))}, seed=180),
        # (19 + 125) x 256 resident values: forward 4 * (4032 + 16 * 44 - 768 + 36864), BPTT 4 * (4032 + 36864) of the 163840 bytes
        Case("lds_full", (2,), (Mem(Lu, 75, 256), Mem(Lu, 500, 256)), 3, 2, 256, 128, Vs=(41,),
             plan={2: _p(1, (19, 125), lds_fwd=163328, lds_bwd=163584)}, seed=190),
        Case("no_finals_no_h0", (0, 2), (Mem(Lu, 37, 32),), 11, 4, 32, 16, plan={0: _p(3, (19,), rows=16), 2: _p(0, (10,))}, h0=False,
             finals=False, seed=200),
    ]
    return C


CASES = _table()
BY_NAME = {c.name: c for c in CASES}


def expected_plan(case, key, fused, bwd):
    """What avsr_attn_rnn_plan must answer for (case, key) under avsr_attn_rnn_set_fused(fused): "per_step" or (dict of fields)."""
    mode, V = key
    p = case.plan[mode]
    on = fused in ((1, 3) if bwd else (1, 2))
    if p is None or not on:
        return "per_step"
    want = dict(form="fused", variant=p["variant"], rows_per_group=p["rows"], quarter=p["quarter"], launches=p["launches"],
                v64=int((not bwd) and mode >= 1 and V > 32))
    lds = p.get("lds_bwd" if bwd else "lds_fwd")
    if lds:
        want["lds_bytes"] = lds
    return want


def plan_matches(rec, want):
    """Does a plan record (ops.attn_rnn_plan) say what expected_plan names?"""
    if want == "per_step":
        return rec["form"] == "per_step" and rec["variant"] == -1 and rec["rows_per_group"] == 0 and rec["lds_bytes"] == 0
    return all(rec.get(k) == v for k, v in want.items())


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def _hold(rng, n, hi, must):
    """n integers in [1, hi] that hold the values `must` (as many of them as n allows, in order)."""
    a = rng.integers(1, hi + 1, size=n).astype(np.int32)
    slots = rng.permutation(n)
    for s, v in zip(slots, must):
        a[s] = min(max(int(v), 1), hi)
    return a


# The draw of (case, mode, V), searched so that the conditions of tests/test_dec_check_cpu.py part (b) hold (no tool is needed: a draw
# that fails them fails that test).  0 where not listed.  The margin a decision must keep is 100 x the case's own logits bound, and the
# noise in that bound is an fp32 run of this machine's torch (it moves by some 10 % between hosts): on the sampling rows whose bound the
# noise decides (scaled_D_ne_H_drop, v33) the draw keeps 2.5 x the margin.
SEEDS = {("scaled_D_ne_H_drop", 2, 32): 2, ("v33", 1, 33): 4, ("v33", 2, 33): 4, ("two_q32", 1, 28): 2, ("two_v2", 1, 28): 7, ("two_v2", 1, 41): 1, ("two_v2", 2, 28): 5,
         ("two_v2", 2, 41): 2, ("dec_b67", 2, 28): 24, ("bahdanau", 2, 28): 9, ("bahdanau", 2, 41): 2, ("normed_bahdanau", 2, 28): 3,
         ("normed_bahdanau", 2, 41): 2}


def make_inputs(case, key, seed=None):
    """Weights in engine layout (fp32), memories, lengths, probes.  The kernel W is [E + A + H][4H] with unit-interleaved gate columns."""
    mode, V = key
    draw = SEEDS.get((case.name, mode, V), 0) if seed is None else seed
    rng = np.random.default_rng([case.seed, mode, V, draw])
    B, L, H, E = case.B, case.L, case.H, case.E
    nm = len(case.mems)
    A, f = nm * H, np.float32
    KW = E + A + H
    d = dict(W=(rng.standard_normal((KW, 4 * H)) * 1.5 / np.sqrt(KW)).astype(f), bias=(rng.standard_normal(4 * H) * 0.1).astype(f))
    wpr = 32 // (case.plan[mode]["rows"] if case.plan[mode] else 8)
    d["mem"] = []
    for M in case.mems:
        ch = (M.T + wpr - 1) // wpr
        m = dict(keys=(rng.standard_normal((B, M.T, H)) * 0.5).astype(f), values=rng.standard_normal((B, M.T, M.D)).astype(f),
                 len=_hold(rng, B, M.T, (M.T, 1, ch, ch + 1)), watt=(rng.standard_normal((H + M.D, H)) / np.sqrt(H + M.D)).astype(f))
        if M.type == "scaled_luong":
            m["g"] = np.array([1.7], f)
        if M.type in ("bahdanau", "normed_bahdanau"):
            m["v"] = (rng.standard_normal(H) * 2.0 / np.sqrt(H)).astype(f)
            m["wq"] = (rng.standard_normal((H, H)) / np.sqrt(H)).astype(f)
            if M.type == "normed_bahdanau":
                m["bq"] = (rng.standard_normal(H) * 0.3).astype(f)
        d["mem"].append(m)
    d["steplen"] = np.full(B, L, np.int32) if mode == 1 else _hold(rng, B, L, (L, 1, (L + 1) // 2))
    d["h0"], d["c0"] = (rng.standard_normal((B, H)) * 0.5).astype(f), (rng.standard_normal((B, H)) * 0.5).astype(f)
    if mode == 0:
        x = (rng.standard_normal((B, L, E)) * np.sqrt(KW / E)).astype(f)
        d["zx"] = (x.astype(np.float64) @ d["W"][:E].astype(np.float64)).astype(f)         # the hoisted product, rounded once
    else:
        O = A if case.oa else H
        d["emb"] = (rng.standard_normal((V, E)) * 0.7).astype(f)
        d["wout"] = (rng.standard_normal((O, V)) * 4.0 / np.sqrt(O)).astype(f)
        d["bout"] = (rng.standard_normal(V) * 0.3).astype(f)
        d["labels"] = rng.integers(0, V, size=(B, L)).astype(np.int32)
        d["xs0"] = np.repeat(d["emb"][GO][None], B, 0)                                      # slot 0 of xs: the caller's dropout(emb[GO])
        if case.drop and mode == 2 and case.drop[0] < 1.0:
            u = uniform01(1234 + case.seed + 1000 * draw, CELL_ID * 4, ((np.arange(B) * L)[:, None] * (E + A) + np.arange(E)[None, :]).astype(np.uint32))
            d["xs0"] = np.where(u < f(case.drop[0]), d["xs0"] / f(case.drop[0]), f(0)).astype(f)
    live = np.arange(L)[None, :] < d["steplen"][:, None]
    d["datt_ext"] = (rng.standard_normal((B, L, A)) * live[:, :, None]).astype(f)
    d["dcell_ext"] = (rng.standard_normal((B, L, H)) * live[:, :, None]).astype(f)
    d["dh_final"], d["dc_final"] = rng.standard_normal((B, H)).astype(f), rng.standard_normal((B, H)).astype(f)
    d["seed"] = 1234 + case.seed + 1000 * draw
    return d


# ---- the reference --------------------------------------------------------------------------------------------------------------------
def _bf16(a):
    return a.to(torch.bfloat16).to(a.dtype)


def _mask(seed, stream, keep, idx, dtype):
    if keep >= 1.0:
        return None
    u = uniform01(seed, stream, np.asarray(idx).astype(np.uint32))
    return torch.tensor((u < np.float32(keep)).astype(np.float64) / keep, dtype=dtype)


def run(case, key, inp, dtype=torch.float64, mut=None, force=None, want_grad=True):
    """One block.  mut: {fault: argument} (tests/test_dec_check_cpu.py part c).  force: {"fed" / "ids": tokens} the fp32 twin follows
    instead of its own draws.  Returns numpy fp64 records in the header's layouts plus "live" [B][L] and the decision margins."""
    mode, V = key
    mut = mut or {}
    B, L, H, E = case.B, case.L, case.H, case.E
    nm = len(case.mems)
    A = nm * H
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    W, bias = t(inp["W"]), t(inp["bias"])
    if "bf16" in mut:
        W = _bf16(W)
    drop = case.drop if mode != 1 else None
    k_in, k_st, k_out = drop if drop else (1.0, 1.0, 1.0)
    seed, cid4 = inp["seed"], CELL_ID * 4
    rows = np.arange(B)
    steplen = inp["steplen"].astype(np.int64).copy()
    h0 = t(inp["h0"] if case.h0 else np.zeros((B, H))).requires_grad_(want_grad)
    c0 = t(inp["c0"] if case.h0 else np.zeros((B, H))).requires_grad_(want_grad)
    mem = []
    for mi, M in enumerate(case.mems):
        m = inp["mem"][mi]
        ln = m["len"].astype(np.int64)
        if mut.get("nbr_len") is not None:
            ln = ln.copy()
            ln[mut["nbr_len"]] = ln[mut["nbr_len"] + 1]
        if "softmax_over_T" in mut:
            ln = np.full(B, M.T)
        ok = torch.tensor(np.arange(M.T)[None, :] < ln[:, None])
        ch = (M.T + 3) // 4
        if "drop_quarter" in mut:                      # the last non-empty quarter of every row is left out of the merge
            q_last = (np.minimum(m["len"], M.T) - 1) // ch
            keep_t = (np.arange(M.T)[None, :] // ch) != q_last[:, None]
            ok = ok & torch.tensor(keep_t | (q_last[:, None] == 0))
        mem.append(dict(keys=t(m["keys"]), values=t(m["values"]), ok=ok, watt=t(m["watt"]), g=float(m["g"][0]) if "g" in m else None,
                        v=t(m["v"]) if "v" in m else None, wq=t(m["wq"]) if "wq" in m else None, bq=t(m["bq"]) if "bq" in m else None,
                        empty=torch.tensor(((np.minimum(m["len"], M.T) + ch - 1) // ch) < 4)))
    if mode == 0:
        zx = t(inp["zx"]).reshape(B, L, 4 * H)
    else:
        emb, wout, bout = t(inp["emb"]), t(inp["wout"]), t(inp["bout"])
        if "bf16" in mut:
            wout = _bf16(wout)
    fed = np.zeros((B, L), np.int64)
    fed[:, 0] = GO
    ids, tok = np.zeros((B, L), np.int64), np.full(B, GO, np.int64)
    xs = [t(inp["xs0"])] if mode == 2 else None
    n_unf = 0
    h, c = h0, c0
    if "h0_at_step1" in mut:
        h = h0 * 0.0
    zero_att = torch.zeros(B, A, dtype=dtype)
    att_prev = attd_prev = zero_att
    S = dict(z=[], gates=[], cs=[], cell_out=[], hs=[], att=[], attd=[], logits=[], live=[], margin=[], edge=[], bern=[])
    R = [dict(raw=[], s=[], ctx=[], pq=[], pm=[], pl=[]) for _ in case.mems]
    for l in range(L):
        valid_np = l < steplen
        valid = torch.tensor(valid_np)[:, None]
        if "h0_at_step1" in mut and l == 1:
            h = h0
        x_att = att_prev if ("undropped_att_fed" in mut or drop is None) else attd_prev
        if mode == 0:
            zin = zx[:, l]
        else:
            x = xs[l] if mode == 2 else emb[torch.tensor(tok)]
            zin = (_bf16(x) if "bf16" in mut else x) @ W[:E]
        hop, aop = (_bf16(h), _bf16(x_att)) if "bf16" in mut else (h, x_att)
        z = zin + aop @ W[E:E + A] + hop @ W[E + A:] + bias
        if want_grad:
            z.retain_grad()
        zz = z.view(B, H, 4)
        gi, gj, gf, go = torch.sigmoid(zz[..., 0]), torch.tanh(zz[..., 1]), torch.sigmoid(zz[..., 2] + 1.0), torch.sigmoid(zz[..., 3])
        c_new = torch.clamp(gf * c + gi * gj, -1.0, 1.0)
        h_new = go * torch.tanh(c_new)
        oidx = (rows * L + l)[:, None] * H + np.arange(H)[None, :]
        m_o = _mask(seed, cid4 + 2, k_out, oidx, dtype)
        m_s = _mask(seed, cid4 + (2 if "state_mask_from_out" in mut else 1), k_st, oidx, dtype)
        ho = h_new * m_o if m_o is not None else h_new
        hs = h_new * m_s if m_s is not None else h_new
        zero = torch.zeros_like(ho)
        cell_out = torch.where(valid, ho, zero)
        if want_grad:
            cell_out.retain_grad()
        if "no_carry" in mut:
            h, c = torch.where(valid, hs, zero), torch.where(valid, c_new, zero)
        else:
            h, c = torch.where(valid, hs, h), torch.where(valid, c_new, c)
        S["z"].append(z)
        S["gates"].append(torch.stack([gi, gj, gf, go], -1))
        S["cs"].append(c_new)
        S["cell_out"].append(cell_out)
        S["hs"].append(torch.where(valid, hs, zero))
        S["live"].append(valid_np.copy())
        # ---- the mechanisms on the emitted cell output ----
        atts, ctxs = [], []
        for mi, (M, m) in enumerate(zip(case.mems, mem)):
            q = cell_out
            if M.type in ("luong", "scaled_luong"):
                raw = torch.einsum("bth,bh->bt", m["keys"], _bf16(q) if "bf16" in mut else q)
                s = raw * (m["g"] if (m["g"] is not None and "no_g" not in mut) else 1.0)
                pq = None
            else:
                pq = q @ m["wq"]
                if want_grad:
                    pq.retain_grad()
                pre = m["keys"] + pq[:, None, :]
                if m["bq"] is not None and "no_bq" not in mut:
                    pre = pre + m["bq"]
                raw = torch.sum(m["v"] * torch.tanh(pre), dim=-1)
                s = raw * 1.0
            if want_grad:
                s.retain_grad()
            sm = torch.where(m["ok"], s, torch.full_like(s, -float("inf")))
            mx = sm.max(dim=1, keepdim=True).values
            if "empty_zero_max" in mut:                  # an empty quarter counted as one frame of score 0 and value 0
                mx = torch.where(m["empty"][:, None], torch.clamp(mx, min=0.0), mx)
            p = torch.exp(sm - mx)
            lsum = p.sum(dim=1, keepdim=True)
            if "empty_zero_max" in mut:
                lsum = lsum + torch.where(m["empty"][:, None], torch.exp(-mx), torch.zeros_like(mx))
            ctx = torch.einsum("bt,btd->bd", p / lsum, m["values"])
            if want_grad:
                ctx.retain_grad()
            ctxs.append(ctx)
            r = R[mi]
            r["raw"].append(raw), r["s"].append(s), r["ctx"].append(ctx), r["pq"].append(pq), r["pm"].append(mx[:, 0]), r["pl"].append(lsum[:, 0])
        for mi, (M, m) in enumerate(zip(case.mems, mem)):
            cx = ctxs[1 - mi] if ("ctx_swap" in mut and nm == 2) else ctxs[mi]
            atts.append(torch.cat([cell_out, cx], dim=-1) @ m["watt"])
        att = torch.where(valid, torch.cat(atts, dim=-1), zero_att)
        if want_grad:
            att.retain_grad()
        iidx = (rows * L + l + 1)[:, None] * (E + A) + E + np.arange(A)[None, :]
        m_i = _mask(seed, cid4, k_in, iidx, dtype)
        attd = att * m_i if m_i is not None else att
        S["att"].append(att)
        S["attd"].append(attd)
        att_prev, attd_prev = att, attd
        # ---- output layer and the next token ----
        if mode >= 1:
            out = att if case.oa else cell_out
            lg = out @ wout + bout
            if "logits_past_steplen" not in mut:
                lg = torch.where(valid, lg, torch.zeros_like(lg))
            S["logits"].append(lg)
            lg32 = lg.detach().numpy().astype(np.float32)
            if mode == 1:
                best = lg32.argmax(axis=1)
                srt = np.sort(lg.detach().numpy().astype(np.float64), axis=1)
                S["margin"].append(np.where(valid_np, srt[:, -1] - srt[:, -2], np.inf) if V > 1 else np.full(B, np.inf))
                if force is not None:
                    best = force["ids_raw"][:, l]
                S.setdefault("ids_raw", []).append(best.copy())
                ids[:, l] = np.where(valid_np, best, 0)
                tok = np.where(valid_np, best, tok)
                hit = valid_np & (best == EOS)
                steplen = np.where(hit, l + 1, steplen)
                n_unf = int((valid_np & ~hit).sum())
            elif l + 1 < L:
                idx = (rows * L + l + (1 if "sample_idx_off" in mut else 0)).astype(np.uint32)
                ub, us = uniform01(seed, 1000, idx), uniform01(seed, 1001, idx)
                nxt = inp["labels"][:, l].astype(np.int64).copy()
                edge = np.full(B, np.inf)
                if case.prob > 0:
                    S["bern"].append(np.abs(ub.astype(np.float64) - case.prob))
                    for b in range(B):
                        if ub[b] < np.float32(case.prob):
                            nxt[b] = categorical_f32(lg32[b], us[b])
                            pr = np.exp(lg32[b].astype(np.float64) - lg32[b].max())
                            edge[b] = np.abs(np.cumsum(pr)[:-1] / pr.sum() - float(us[b])).min() if V > 1 else np.inf
                S["edge"].append(edge)
                if force is not None:
                    nxt = force["fed"][:, l + 1]
                fed[:, l + 1] = nxt
                xe = emb[torch.tensor(nxt)]
                xidx = (rows * L + l + 1)[:, None] * (E + A) + np.arange(E)[None, :]
                m_x = _mask(seed, cid4, k_in, xidx, dtype)
                xs.append(xe * m_x if m_x is not None else xe)
    # ---- the probe and its gradients ----
    live = np.stack(S["live"], 1)
    res = dict(live=live, steplen=steplen.copy(), h_final=h.detach().numpy().astype(np.float64), c_final=c.detach().numpy().astype(np.float64))
    if want_grad and mode != 1:
        loss = torch.zeros((), dtype=dtype)
        de, dc_ = t(inp["datt_ext"]), t(inp["dcell_ext"])
        for l in range(L):
            loss = loss + (de[:, l] * S["att"][l]).sum() + (dc_[:, l] * S["cell_out"][l]).sum()
        if case.finals:
            sel = torch.tensor((inp["steplen"] == L).astype(np.float64), dtype=dtype)[:, None] if "dh_at_L" in mut else 1.0
            loss = loss + (t(inp["dh_final"]) * h * sel).sum() + (t(inp["dc_final"]) * c * sel).sum()
        loss.backward()
    npy = lambda x: x.detach().numpy().astype(np.float64)
    stack = lambda xs_, shape: np.stack([npy(x) for x in xs_], 1).reshape(shape)
    g_of = lambda xs_, shape: np.stack([npy(x.grad) if x.grad is not None else np.zeros(tuple(x.shape)) for x in xs_], 1).reshape(shape)
    res["gates"], res["cs"] = stack(S["gates"], (B, L, H, 4)), stack(S["cs"], (B, L, H))
    first = npy(h0) if "h0_at_step1" not in mut else np.zeros((B, H))
    res["cell_out"] = np.concatenate([first[:, None], stack(S["cell_out"], (B, L, H))], 1)
    res["hs_seq"] = np.concatenate([first[:, None], stack(S["hs"], (B, L, H))], 1)
    res["att"] = np.concatenate([np.zeros((B, 1, A)), stack(S["att"], (B, L, A))], 1)
    res["attd"] = np.concatenate([np.zeros((B, 1, A)), stack(S["attd"], (B, L, A))], 1)
    res["mem"] = []
    for mi, M in enumerate(case.mems):
        r = R[mi]
        o = dict(scores=stack(r["raw"], (B, L, M.T)), ctx=stack(r["ctx"], (B, L, M.D)), lse=stack(r["pm"], (B, L)) + np.log(stack(r["pl"], (B, L))))
        if r["pq"][0] is not None:
            o["pq"] = stack(r["pq"], (B, L, H))
        if want_grad and mode != 1:
            o["dscores"], o["dctx"] = g_of(r["s"], (B, L, M.T)), g_of(r["ctx"], (B, L, M.D))
            if r["pq"][0] is not None:
                o["dpq"] = g_of(r["pq"], (B, L, H))
        res["mem"].append(o)
    if mode >= 1:
        res["logits"] = stack(S["logits"], (B, L, V))
    if mode == 1:
        res["ids"], res["tok"], res["n_unfinished"] = ids, tok, n_unf
        res["ids_raw"] = np.stack(S["ids_raw"], 1)
        res["margin"] = float(np.min(S["margin"])) if S["margin"] else np.inf
    if mode == 2:
        res["fed"], res["xs"] = fed, stack(xs, (B, L, E))
        res["edge"] = float(np.min(S["edge"])) if S["edge"] else np.inf
        res["bern"] = float(np.min(S["bern"])) if S["bern"] else np.inf
    if want_grad and mode != 1:
        res["dgates"] = g_of(S["z"], (B, L, H, 4))
        res["datt"] = g_of(S["att"], (B, L, A))
        res["dh0"], res["dc0"] = npy(h0.grad) if h0.grad is not None else np.zeros((B, H)), npy(c0.grad) if c0.grad is not None else np.zeros((B, H))
    return res


FWD_Q = ("gates", "cs", "cell_out", "hs_seq", "att", "attd", "logits", "xs", "h_final", "c_final")
BWD_Q = ("dgates", "datt", "dh0", "dc0")
MEM_FWD_Q = ("scores", "ctx", "lse", "pq")
MEM_BWD_Q = ("dscores", "dctx", "dpq")


def noise_of(r64, r32):
    """Per quantity: (largest |fp32 twin - fp64|, largest |fp64| entry) over the live entries of a case."""
    out = {}
    for q in FWD_Q + BWD_Q:
        if q in r64:
            out[q] = (float(np.abs(r64[q] - r32[q]).max(initial=0.0)), float(np.abs(r64[q]).max(initial=0.0)))
    live = r64["live"]
    for q in MEM_FWD_Q + MEM_BWD_Q:
        gap = big = 0.0
        for a, b in zip(r64["mem"], r32["mem"]):
            if q in a:
                w = live.reshape(live.shape + (1,) * (a[q].ndim - 2))
                fin = np.isfinite(a[q]) & w
                gap = max(gap, float(np.abs(np.where(fin, a[q] - b[q], 0.0)).max(initial=0.0)))
                big = max(big, float(np.abs(np.where(fin, a[q], 0.0)).max(initial=0.0)))
        if any(q in a for a in r64["mem"]):
            out[q] = (gap, big)
    return out


_CACHE = {}


def fixture(case, key):
    """(inputs, fp64 reference, noise) of (case, key), computed once per process and never modified by its users."""
    k = (case.name,) + tuple(key)
    if k not in _CACHE:
        inp = make_inputs(case, key)
        r64 = run(case, key, inp)
        force = dict(fed=r64.get("fed"), ids_raw=r64.get("ids_raw"))
        _CACHE[k] = (inp, r64, noise_of(r64, run(case, key, inp, torch.float32, force=force)))
    return _CACHE[k]


def tolerance(q, noise, ref_max=0.0):
    """max(T_suite, 8 x noise): the rule of the recurrent suite."""
    t = T_SUITE_BPTT * max(1.0, ref_max) if q.startswith("d") else T_SUITE
    return max(t, 8.0 * noise[q][0])


def conditions(case, key, ref, noise):
    """What tests/test_dec_check_cpu.py part (b) asks of the inputs, measured on the reference alone."""
    rel = max(v[0] / v[1] for v in noise.values() if v[1] > 0)
    return dict(noise_rel=rel, margin=ref.get("margin", np.inf), edge=ref.get("edge", np.inf), bern=ref.get("bern", np.inf))


BERN_MARGIN = 1e-3


def margin_of(noise):
    """What a decision of a case must keep clear: MARGIN_FACTOR x the case's own logits bound max(T_suite, 8 x noise)."""
    return MARGIN_FACTOR * tolerance("logits", noise) if "logits" in noise else MARGIN_FACTOR * T_SUITE


def holds(case, key, inp, ref, noise):
    """The conditions on the decisions of a case (every element counts): each greedy argmax leads by margin_of(noise), each sampling
    uniform keeps that far from the edges of its CDF bin, each select draw BERN_MARGIN from sampling_prob; a greedy case of 20 or more
    (row, step) pairs has a row that emits EOS early and one that never does; a sampling case feeds at least one token that is not the
    label."""
    mode, V = key
    m = margin_of(noise)
    ok = ref.get("margin", np.inf) >= m and ref.get("edge", np.inf) >= m and ref.get("bern", np.inf) >= BERN_MARGIN
    if mode == 1 and case.B * case.L >= 20:
        ok = ok and bool((ref["steplen"] < case.L).any()) and ref["n_unfinished"] > 0
    if mode == 2 and case.prob > 0:
        ok = ok and bool((ref["fed"][:, 1:] != inp["labels"][:, :case.L - 1]).any())
    return bool(ok)


# ---- the engine's buffers -------------------------------------------------------------------------------------------------------------
F32, I32 = "f", "i"


def layout(case, key):
    """Every buffer of a call as {name: (elements, dtype, kind)}; kind: "in" (bit-unchanged), "out" (judged), "scratch" (bands only)."""
    mode, V = key
    B, L, H, E = case.B, case.L, case.H, case.E
    nm = len(case.mems)
    A, KW = nm * H, E + nm * H + H
    drop = case.drop and mode != 1
    Lo = {"wt": (4 * H * KW, F32, "in"), "w": (KW * 4 * H, F32, "in"), "bias": (4 * H, F32, "in"), "seed": (1, I32, "in"),
          "steplen": (B, I32, "out" if mode == 1 else "in"),
          "gates": (B * L * H * 4, F32, "out"), "cs": (B * L * H, F32, "out"), "cell_out": (B * (L + 1) * H, F32, "out"),
          "att": (B * (L + 1) * A, F32, "out"), "state": (4 * B * H, F32, "scratch"), "fused_ws": (fused_ws_floats(B, nm), F32, "scratch")}
    if case.h0:
        Lo["h0"], Lo["c0"] = (B * H, F32, "in"), (B * H, F32, "in")
    if mode != 1:
        Lo["h_final"], Lo["c_final"] = (B * H, F32, "out"), (B * H, F32, "out")
        Lo.update({"dgates": (B * L * H * 4, F32, "out"), "dstate": (12 * B * H, F32, "scratch"), "datt": (B * L * A, F32, "out"),
                   "dq": (B * L * H, F32, "scratch"), "datt_ext": (B * L * A, F32, "in"), "dcell_ext": (B * L * H, F32, "in"),
                   "dh0": (B * H, F32, "out"), "dc0": (B * H, F32, "out")})
        if case.finals:
            Lo["dh_final"], Lo["dc_final"] = (B * H, F32, "in"), (B * H, F32, "in")
    if drop:
        Lo["hs_seq"], Lo["attd"] = (B * (L + 1) * H, F32, "out"), (B * (L + 1) * A, F32, "out")
    if mode >= 1:
        O = A if case.oa else H
        Lo.update({"embedding": (V * E, F32, "in"), "wout_t": (V * O, F32, "in"), "bout": (V, F32, "in"), "logits": (B * L * V, F32, "out")})
    if mode == 1:
        Lo.update({"ids": (B * L, I32, "out"), "tok": (B, I32, "out"), "n_unfinished": (1, I32, "out")})
    if mode == 2:
        Lo.update({"xs": (B * L * E, F32, "out"), "labels": (B * L, I32, "in"), "fed": (B * L, I32, "out")})
    for mi, M in enumerate(case.mems):
        k = lambda n: "%s%d" % (n, mi)
        Lo.update({k("len"): (B, I32, "in"), k("keys"): (B * M.T * H, F32, "in"), k("values"): (B * M.T * M.D, F32, "in"),
                   k("watt_t"): (H * (H + M.D), F32, "in"), k("watt"): ((H + M.D) * H, F32, "in"),
                   k("scores"): (B * L * M.T, F32, "out"), k("ctx"): (B * L * M.D, F32, "out"), k("pstat"): (L * 2 * M.nchunk * B, F32, "out"),
                   k("pctx"): (M.nchunk * B * M.D, F32, "scratch")})
        if M.type == "scaled_luong":
            Lo[k("g")] = (1, F32, "in")
        if M.type in ("bahdanau", "normed_bahdanau"):
            Lo.update({k("v"): (H, F32, "in"), k("wq_t"): (H * H, F32, "in"), k("wq"): (H * H, F32, "in"), k("pq"): (B * L * H, F32, "out")})
            if M.type == "normed_bahdanau":
                Lo[k("bq")] = (H, F32, "in")
        if mode != 1:
            Lo.update({k("dscores"): (B * L * M.T, F32, "out"), k("dctx"): (B * L * M.D, F32, "out"), k("pdq"): (M.nchunk * B * H, F32, "scratch")})
            if M.type in ("bahdanau", "normed_bahdanau"):
                Lo[k("dpq")] = (B * L * H, F32, "out")
    return Lo


def fused_ws_floats(B, n_mech):
    """avsr_attn_rnn_fused_ws_floats(B, n_mech, 256), restated (include/avsr_hip.h; the GPU test asserts the library agrees)."""
    fwd = ((B + 7) // 8 + 16) * 32 * 8 * 64 + n_mech * (8 * B + 4 * B * 256) + 64
    bwd = ((B + 15) // 16) * 16 * 32 * 512 + n_mech * 4 * B * 256
    return fwd + bwd


def alloc(n):
    a = np.empty(n + 2 * GUARD, np.float32)
    a.view(np.uint32)[:] = PATTERN
    return a


def inner(a):
    return a[GUARD:len(a) - GUARD]


def iview(a):
    return inner(a).view(np.int32)


def initial_buffers(case, key, inp):
    """The buffers as the caller hands them over, each inside its NaN band: inputs filled, everything a call writes (and every slot or row
    it must leave alone) NaN pattern; in mode 1 the caller zeroes ids and logits (a group that has finished stops writing)."""
    mode, V = key
    B, L, H, E = case.B, case.L, case.H, case.E
    nm = len(case.mems)
    A = nm * H
    bufs = {k: alloc(n) for k, (n, _t, _k) in layout(case, key).items()}
    put = lambda k, a: inner(bufs[k]).__setitem__(slice(None), np.asarray(a, np.float32).reshape(-1))
    puti = lambda k, a: iview(bufs[k]).__setitem__(slice(None), np.asarray(a, np.int32).reshape(-1))
    put("w", inp["W"]), put("wt", inp["W"].T), put("bias", inp["bias"]), puti("seed", [inp["seed"]]), puti("steplen", inp["steplen"])
    if case.h0:
        put("h0", inp["h0"]), put("c0", inp["c0"])
    if mode == 0:
        put("gates", inp["zx"])
    if mode != 1:
        put("datt_ext", inp["datt_ext"]), put("dcell_ext", inp["dcell_ext"])
        if case.finals:
            put("dh_final", inp["dh_final"]), put("dc_final", inp["dc_final"])
    if mode >= 1:
        put("embedding", inp["emb"]), put("wout_t", inp["wout"].T), put("bout", inp["bout"])
    if mode == 1:
        puti("ids", np.zeros(B * L)), put("logits", np.zeros(B * L * V)), puti("tok", np.full(B, GO))
    if mode == 2:
        puti("labels", inp["labels"])
        iview(bufs["fed"]).reshape(B, L)[:, 0] = GO
        inner(bufs["xs"]).reshape(B, L, E)[:, 0] = inp["xs0"]
    for mi, M in enumerate(case.mems):
        m = inp["mem"][mi]
        k = lambda n: "%s%d" % (n, mi)
        puti(k("len"), m["len"]), put(k("keys"), m["keys"]), put(k("values"), m["values"]), put(k("watt"), m["watt"]), put(k("watt_t"), m["watt"].T)
        for n in ("g", "v", "bq"):
            if n in m:
                put(k(n), m[n])
        if "wq" in m:
            put(k("wq"), m["wq"]), put(k("wq_t"), m["wq"].T)
    return bufs


def mem_pstat(buf, case, mi):
    """Merged softmax statistics of a pstat buffer [L][2][nchunk][B] as log-sum-exp [B][L] (a form may record them per chunk or merged)."""
    M = case.mems[mi]
    p = inner(buf).astype(np.float64).reshape(case.L, 2, M.nchunk, case.B)
    pm, pl = p[:, 0], p[:, 1]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mx = pm.max(axis=1)
        s = np.where(np.isneginf(pm), 0.0, np.exp(pm - mx[:, None]) * pl).sum(axis=1)
        return (mx + np.log(s)).T


def set_pstat(buf, case, mi, lse):
    """Write merged statistics into chunk 0 of a pstat buffer, neutral elsewhere (what the fused kernel leaves)."""
    M = case.mems[mi]
    p = inner(buf).reshape(case.L, 2, M.nchunk, case.B)
    p[:, 0], p[:, 1] = -np.inf, 0.0
    p[:, 0, 0], p[:, 1, 0] = lse.T, 1.0


def expected_buffers(case, key, inp, ref):
    """The buffers as a correct engine leaves them after forward + BPTT, built from the reference (the CPU side of the checker's tests
    mutates copies of these).  Entries the contract leaves unspecified keep their fill."""
    mode, V = key
    B, L, H, E = case.B, case.L, case.H, case.E
    A = len(case.mems) * H
    bufs = initial_buffers(case, key, inp)
    live = ref["live"]
    v = lambda k, shape: inner(bufs[k]).reshape(shape)
    v("gates", (B, L, H, 4))[live] = ref["gates"][live]
    v("cs", (B, L, H))[live] = ref["cs"][live]
    full = np.concatenate([np.ones((B, 1), bool), live | (mode != 1)], 1)          # mode 1: dead slots are unspecified
    for k, W_ in (("cell_out", H), ("att", A), ("hs_seq", H), ("attd", A)):
        if k in bufs:
            v(k, (B, L + 1, W_))[full] = ref[k][full]
    if mode != 1:
        v("h_final", (B, H))[:], v("c_final", (B, H))[:] = ref["h_final"], ref["c_final"]
        v("dgates", (B, L, H, 4))[:], v("datt", (B, L, A))[:] = ref["dgates"], ref["datt"]
        v("dh0", (B, H))[:], v("dc0", (B, H))[:] = ref["dh0"], ref["dc0"]
    if mode >= 1:
        v("logits", (B, L, V))[:] = ref["logits"]
    if mode == 1:
        iview(bufs["ids"])[:], iview(bufs["tok"])[:], iview(bufs["steplen"])[:] = ref["ids"].reshape(-1), ref["tok"], ref["steplen"]
        iview(bufs["n_unfinished"])[:] = ref["n_unfinished"]
    if mode == 2:
        iview(bufs["fed"])[:] = ref["fed"].reshape(-1)
        v("xs", (B, L, E))[:, 1:] = ref["xs"][:, 1:]
    for mi, M in enumerate(case.mems):
        r = ref["mem"][mi]
        k = lambda n: "%s%d" % (n, mi)
        inl = (np.arange(M.T)[None, :] < inp["mem"][mi]["len"][:, None])
        sc = v(k("scores"), (B, L, M.T))
        m3 = live[:, :, None] & inl[:, None, :]
        sc[m3] = r["scores"][m3]
        v(k("ctx"), (B, L, M.D))[live] = r["ctx"][live]
        set_pstat(bufs[k("pstat")], case, mi, np.where(live, r["lse"], 0.0))
        if "pq" in r:
            v(k("pq"), (B, L, H))[live] = r["pq"][live]
        if mode != 1:
            v(k("dscores"), (B, L, M.T))[:], v(k("dctx"), (B, L, M.D))[:] = r["dscores"], r["dctx"]
            if "dpq" in r:
                v(k("dpq"), (B, L, H))[:] = r["dpq"]
    return bufs


# ---- the checker ----------------------------------------------------------------------------------------------------------------------
def _first(bad):
    idx = np.argwhere(bad)
    return tuple(int(i) for i in idx[0]) if len(idx) else None


def _bits(a):
    return a.view(np.uint32)


def check(case, key, inp, ref, noise, before, after, again=None, split=None, err_word=0, log=None):
    """Judge the engine's buffers `after` a forward (+ BPTT outside mode 1) on `before` against the reference.  Returns None or the first
    offence as (buffer, index..., what).  again: the buffers of a second identical call, split: those of a run whose forward was issued
    as [0, 2) then [2, L) -- both must be bit-equal to `after` outside the scratch.  log receives (quantity, largest error, bound)."""
    mode, V = key
    B, L, H, E = case.B, case.L, case.H, case.E
    A = len(case.mems) * H
    Lo = layout(case, key)
    if err_word != 0:
        return ("sync", "sticky error word %d" % err_word)
    for k in before:                                    # the NaN band around every buffer, fused_ws' surroundings included
        for part, sl in (("low", slice(0, GUARD)), ("high", slice(-GUARD, None))):
            bad = _bits(after[k])[sl] != PATTERN
            if bad.any():
                return (k, "wrote %s guard band at word %d" % (part, _first(bad)[0]))
    for k, (_n, _t, kind) in Lo.items():               # inputs
        if kind == "in" and not (_bits(after[k]) == _bits(before[k])).all():
            return (k, "the call wrote its input at word %d" % (_first(_bits(after[k]) != _bits(before[k]))[0] - GUARD))
    live = ref["live"]
    dead = ~live
    g = lambda k, shape: inner(after[k]).reshape(shape)
    g0 = lambda k, shape: inner(before[k]).reshape(shape)

    def cmp(name, q, got, want, mask, bptt=False):
        tol = tolerance(q, noise, float(np.abs(want).max(initial=0.0)) if bptt else 0.0)
        mask = np.broadcast_to(mask, got.shape)
        gap = np.where(mask, np.abs(got.astype(np.float64) - np.where(mask, want, 0.0)), 0.0)
        gap = np.where(mask & ~np.isfinite(got), np.inf, gap)
        if log is not None:
            log.append((q, float(gap.max(initial=0.0)), tol))
        f = _first(gap > tol)
        return None if f is None else (name,) + f + ("got %r want %r (bound %.3g)" % (float(got[f]), float(want[f]), tol),)

    def same(name, got, orig, mask, what):
        f = _first((_bits(got) != _bits(orig)) & np.broadcast_to(mask, got.shape))
        return None if f is None else (name,) + f + (what + ": %r" % float(got[f]),)

    def zero(name, got, mask, what):
        f = _first(((_bits(got) & np.uint32(0x7FFFFFFF)) != 0) & np.broadcast_to(mask, got.shape))
        return None if f is None else (name,) + f + (what + ": %r" % float(got[f]),)

    checks = []
    # records of live steps; rows of dead steps are not written
    for k, shape in (("gates", (B, L, H, 4)), ("cs", (B, L, H))):
        w = live.reshape((B, L) + (1,) * (len(shape) - 2))
        checks.append(lambda k=k, shape=shape, w=w: cmp(k, k, g(k, shape), ref[k], w))
        checks.append(lambda k=k, shape=shape, w=w: same(k, g(k, shape), g0(k, shape), ~w, "a dead step's row was written"))
    # slot-padded sequences: slot 0 written by the call, live slots compared, dead slots exact zeros (mode 1: zero or untouched)
    for k, W_ in (("cell_out", H), ("att", A), ("hs_seq", H), ("attd", A)):
        if k not in after:
            continue
        got = g(k, (B, L + 1, W_))
        checks.append(lambda k=k, got=got: zero(k, got[:, :1] - ref[k][:, :1].astype(np.float32), True, "slot 0 is not the initial value"))
        checks.append(lambda k=k, got=got: cmp(k, k, got[:, 1:], ref[k][:, 1:], live[:, :, None]))
        if mode != 1:
            checks.append(lambda k=k, got=got: zero(k, got[:, 1:], dead[:, :, None], "not zero at a dead step"))
        else:           # greedy: a group whose rows have all finished stops, so a dead slot holds a zero or was never written
            checks.append(lambda k=k, got=got: zero(k, got[:, 1:], dead[:, :, None] & (_bits(got[:, 1:]) != PATTERN),
                                                    "neither zero nor untouched at a dead step"))
    if mode != 1:
        for k in ("h_final", "c_final"):
            checks.append(lambda k=k: cmp(k, k, g(k, (B, H)), ref[k], True))
    if mode >= 1:
        checks.append(lambda: cmp("logits", "logits", g("logits", (B, L, V)), ref["logits"], live[:, :, None]))
        checks.append(lambda: zero("logits", g("logits", (B, L, V)), dead[:, :, None], "not zero at a dead step"))
    # tokens: exact, no element left out
    ints = []
    if mode == 1:
        ints = [("ids", ref["ids"].reshape(-1)), ("tok", ref["tok"]), ("steplen", ref["steplen"]), ("n_unfinished", np.array([ref["n_unfinished"]]))]
    if mode == 2:
        ints = [("fed", ref["fed"].reshape(-1))]
        checks.append(lambda: cmp("xs", "xs", g("xs", (B, L, E))[:, 1:], ref["xs"][:, 1:], True))
        checks.append(lambda: same("xs", g("xs", (B, L, E))[:, :1], g0("xs", (B, L, E))[:, :1], True, "slot 0 (the caller's) was written"))
    for k, want in ints:
        checks.append(lambda k=k, want=want: None if (iview(after[k]) == want).all() else
                      (k, _first(iview(after[k]) != want)[0], "got %d want %d" % (iview(after[k])[_first(iview(after[k]) != want)[0]],
                                                                                  want[_first(iview(after[k]) != want)[0]])))
    for mi, M in enumerate(case.mems):
        r = ref["mem"][mi]
        kk = lambda n: "%s%d" % (n, mi)
        inl = (np.arange(M.T)[None, :] < inp["mem"][mi]["len"][:, None])[:, None, :]
        l3 = live[:, :, None]
        sc = g(kk("scores"), (B, L, M.T))
        checks.append(lambda sc=sc, r=r, n=kk("scores"), inl=inl: cmp(n, "scores", sc, r["scores"], l3 & inl))
        checks.append(lambda sc=sc, n=kk("scores"), inl=inl, mi=mi, M=M: same(n, sc, g0(n, (B, L, M.T)), ~inl, "a frame at t >= len was written"))
        checks.append(lambda r=r, n=kk("ctx"), M=M: cmp(n, "ctx", g(n, (B, L, M.D)), r["ctx"], l3))
        checks.append(lambda r=r, n=kk("pstat"), mi=mi: cmp(n, "lse", mem_pstat(after[n], case, mi), r["lse"], live))
        if "pq" in r:
            checks.append(lambda r=r, n=kk("pq"): cmp(n, "pq", g(n, (B, L, H)), r["pq"], l3))
        if mode != 1:
            ds = g(kk("dscores"), (B, L, M.T))
            checks.append(lambda ds=ds, r=r, n=kk("dscores"): cmp(n, "dscores", ds, r["dscores"], True, bptt=True))
            checks.append(lambda ds=ds, n=kk("dscores"), inl=inl: zero(n, ds, ~inl | dead[:, :, None], "not zero at t >= len or a dead step"))
            checks.append(lambda r=r, n=kk("dctx"), M=M: cmp(n, "dctx", g(n, (B, L, M.D)), r["dctx"], True, bptt=True))
            if "dpq" in r:
                checks.append(lambda r=r, n=kk("dpq"): cmp(n, "dpq", g(n, (B, L, H)), r["dpq"], True, bptt=True))
    if mode != 1:
        checks.append(lambda: cmp("dgates", "dgates", g("dgates", (B, L, H, 4)), ref["dgates"], True, bptt=True))
        checks.append(lambda: zero("dgates", g("dgates", (B, L, H, 4)), dead[:, :, None, None], "not zero at a dead step"))
        checks.append(lambda: cmp("datt", "datt", g("datt", (B, L, A)), ref["datt"], True, bptt=True))
        checks.append(lambda: cmp("dh0", "dh0", g("dh0", (B, H)), ref["dh0"], True, bptt=True))
        checks.append(lambda: cmp("dc0", "dc0", g("dc0", (B, H)), ref["dc0"], True, bptt=True))
    for c in checks:
        bad = c()
        if bad:
            return bad
    for what, other in (("second identical call", again), ("forward split at step 2", split)):
        if other is None:
            continue
        for k, (_n, _t, kind) in Lo.items():
            if kind == "scratch":
                continue
            d = _bits(after[k]) != _bits(other[k])
            if d.any():
                return (k, "%s differs at word %d" % (what, _first(d)[0] - GUARD))
    return None


# ---- descriptors ----------------------------------------------------------------------------------------------------------------------
def descriptor(case, key, addr, with_ws=True):
    """The AttnRnn descriptor of (case, key).  addr(name) -> address of the first element of that buffer (past its guard band)."""
    from avsr_tf1_amd._lib import AttnRnn
    mode, V = key
    B, L, H, E = case.B, case.L, case.H, case.E
    Lo = layout(case, key)
    a = lambda n: addr(n) if n in Lo else None
    d = AttnRnn()
    d.B, d.L, d.H, d.E, d.n_mech, d.output_attention, d.V, d.mode = B, L, H, E, len(case.mems), case.oa, V, mode
    d.go_id, d.eos_id, d.prof_tag = GO, EOS, case.prof_tag
    for n in ("steplen", "wt", "w", "bias", "gates", "cs", "cell_out", "att", "h0", "c0", "state", "h_final", "c_final", "embedding", "wout_t",
              "bout", "logits", "ids", "tok", "n_unfinished", "dgates", "dstate", "datt", "dq", "datt_ext", "dcell_ext", "dh0", "dc0",
              "dh_final", "dc_final", "seed", "hs_seq", "attd", "xs", "labels", "fed"):
        setattr(d, n, a(n))
    if case.drop and mode != 1:
        d.keep_in, d.keep_state, d.keep_out = case.drop
    else:
        d.keep_in = d.keep_state = d.keep_out = 1.0
    d.sampling_prob, d.cell_id = (case.prob if mode == 2 else 0.0), CELL_ID
    for mi, M in enumerate(case.mems):
        X = d.mech[mi]
        X.type, X.T, X.D, X.chunk = TYPES.index(M.type), M.T, M.D, M.chunk
        X.values_sb, X.values_st = M.T * M.D, M.D
        for n in ("len", "keys", "values", "g", "v", "bq", "wq_t", "wq", "watt_t", "watt", "scores", "ctx", "pq", "pstat", "pctx", "dscores",
                  "dctx", "dpq", "pdq"):
            setattr(X, n, a("%s%d" % (n, mi)))
    if with_ws:
        d.fused_ws, d.fused_ws_floats = addr("fused_ws"), Lo["fused_ws"][0]
    return d


def plan(case, key, fused, bwd):
    """ops.attn_rnn_plan of (case, key) under avsr_attn_rnn_set_fused(fused) with a sync scratch registered.  No GPU: every pointer is one
    dummy address (the plan never dereferences one); the setting and the registration are put back."""
    from avsr_tf1_amd import ops
    from avsr_tf1_amd.ops import _L
    try:
        _L().avsr_rnn_set_persistent(64, 1 << 20)
        ops.attn_rnn_set_fused(fused)
        return ops.attn_rnn_plan(descriptor(case, key, lambda n: 64), bwd=bwd)
    finally:
        ops.attn_rnn_set_fused(1)
        _L().avsr_rnn_set_persistent(None, 0)
