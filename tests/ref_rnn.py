"""Reference, case table and checker of the encoder RNN conformance suite (tests/test_rnn_check_cpu.py judges them on the CPU,
tests/test_gpu_rnn_conformance.py runs avsr_rnn_fwd / avsr_rnn_bwd against them).  A plain helper module, not a conftest.

The reference restates the semantics of include/avsr_hip.h ("Multi-layer masked RNN over a sequence") as an explicit time loop:
  * for t >= len[b] the output row is zero and the state is carried through; reverse walks len-1 .. 0 and stores at the original
    positions; the LSTM has forget bias 1 and cell clip +-1, gate order i, j, f, o; GRU and ResidualWrapper layers as the header has them;
  * DropoutWrapper masks are oracle.hash_u32 / uniform01 bits with stream = cell_id*4 + {0 in, 1 state, 2 out}, cell_id = cell_id_base +
    layer, index = (b*T + t)*width + column;
  * everything is in ENGINE layout: LSTM gate columns are unit-interleaved (4*unit + {i, j, f, o}), GRU gate columns 2*unit + {r, u};
  * the hoisted product x.Wx of layer 0 is an INPUT (computed in fp64, rounded once to fp32: what the engine finds in `gates`), so no GEMM
    is part of the suite, and `dgates` = d(loss)/d(pre-activation) is compared directly (no deferred weight-gradient GEMM either);
  * the backward is autograd of a random linear probe on the top outputs, the top final h and c (unless the case passes them as NULL)
    and, with dropout, the xt_seq the consumer of the top layer sees.
The same function at torch.float32 is the fp32 twin whose distance from the fp64 run is the `noise` of a case."""
import dataclasses
from typing import Optional, Tuple

import numpy as np
import torch

from oracle.avsr_oracle import uniform01

T_SUITE = 2e-5              # gates, cs, outputs, final states: tests/test_gpu_kernels.py::test_rnn_stack_fwd_bwd
T_SUITE_DGATES = 2e-4       # x max(1, max|ref|): the same test's bound on what it derives from dgates
NOISE_CAP = 1.25e-5         # relative noise a case may have (tests/test_regime_cpu.py)
GUARD = 64                  # floats of NaN pattern on either side of every buffer
PATTERN = np.uint32(0x7FC0BEEF)      # a quiet NaN with a recognisable payload
F_IN = 20                   # feature width under the hoisted layer (only the row stride in+H of its kernel depends on it)
Z0_STD = 2.5                # the input features are scaled so that the hoisted product x.Wx has this standard deviation at every width: the
                            # layers above see inputs inside (-1, 1), so layer 0 is where a case gets its saturated gates and clipped cells


# ---- the case table -------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Drop:
    keep_in: float = 0.8
    keep_state: float = 0.9
    keep_out: float = 0.7
    consumer_keep: float = 0.8
    consumer_stream: int = 77
    seed: int = 1234


@dataclasses.dataclass(frozen=True)
class Stack:
    units: Tuple[int, ...]
    T: int
    reverse: int = 0
    cell: str = "lstm"
    residual: Tuple[int, ...] = ()          # layers wrapped in a ResidualWrapper
    lens: str = "std"                       # "std": holds T, 1 and 0; "null": len == NULL; "alt": another draw that holds T, 1 and 0;
                                            # "short": T, 1, 0 and otherwise at most 2 (a wide stack at B > 64 has too many cell states for
                                            # none of them to lie within 1e-4 of the clip)
    drop: Optional[Drop] = None
    finals: bool = True                     # dh_final / dc_final given (False: NULL)
    share: Optional[Tuple[int, int, int]] = None     # top layer writes (buffer id, ld_out, out_col) and reads dout the same way
    cell_id_base: int = 3


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    B: int
    stacks: Tuple[Stack, ...]
    fwd: dict            # mode -> expected forward plan: form, or (form, {field: value}); a list = one record per stack
    bwd: dict            # mode -> expected BPTT plan
    seed: int = 0
    modes: Tuple[int, ...] = (0, 1, 3, 6)
    small_scratch: bool = False     # also run mode 3 with a K-split scratch that is too small: the plan must say unit-partitioned
    clips: bool = True              # False: T == 1, a cell cannot clip on its first step (|i * j| < 1)


PS = "per_step"


def _both(name, B, units, T, fwd, bwd, seed, **kw):
    """One row of the table, forward and reverse.  seed: one per direction, searched so that the conditions of
    tests/test_rnn_check_cpu.py part (b) hold (tools are not needed: any seed that fails them fails that test)."""
    extra = {k: kw.pop(k) for k in ("modes", "small_scratch", "clips") if k in kw}
    return [Case("%s/%s" % (name, "rv" if r else "fw"), B, (Stack(units, T, reverse=r, **kw),), fwd, bwd, seed[r], **extra) for r in (0, 1)]


def _lstm_modes(fwd3, fwd1, bwd3, bwd6):
    return {0: PS, 1: fwd1, 3: fwd3, 6: fwd3}, {0: PS, 1: PS, 3: bwd3, 6: bwd6}


def _table():
    C = []
    # 8-unit hoisted layer (uw = 8), K tails of 8 and 24; BPTT declined (H % 16): per-step BPTT after a persistent forward
    f, b = _lstm_modes(("fwd_xcd8", dict(wg_per_xcd=9, launches=1)), "fwd_agent", PS, PS)
    C += _both("u8_24_40", 11, (8, 24, 40), 7, f, b, (2100, 1101))
    # forward <8>, K-split (cost 12, no crossing edge), unit-partitioned with a two-tile top (cost 6), agent-scope forward
    f, b = _lstm_modes(("fwd_xcd8", dict(wg_per_xcd=12)), "fwd_agent", ("bwd_ksplit", dict(wg_per_xcd=12, crossing_edges=0, launches=1)),
                       ("bwd_unit", dict(wg_per_xcd=6, top_tiles=2, crossing_edges=0, launches=1)))
    C += _both("u32_48_32_b19", 19, (32, 48, 32), 8, f, b, (110, 111), small_scratch=True)
    # forward <16> (last group 6 rows), solo K-split, unit-partitioned slices 64 + 6
    f, b = _lstm_modes(("fwd_xcd16", dict(rows_per_group=16, launches=1)), "fwd_agent", ("bwd_ksplit_solo", dict(launches=1)),
                       ("bwd_unit", dict(launches=2, rows_per_slice=64)))
    C += _both("u32_48_32_b70", 70, (32, 48, 32), 8, f, b, (120, 2121))
    # forward slices 128 + 3, solo K-split 128 + 3, unit-partitioned 64 + 64 + 3
    f, b = _lstm_modes(("fwd_xcd16", dict(launches=2, rows_per_slice=128)), "fwd_agent", ("bwd_ksplit_solo", dict(launches=2, rows_per_slice=128)),
                       ("bwd_unit", dict(launches=3)))
    C += _both("u32_48_32_b131", 131, (32, 48, 32), 3, f, b, (3130, 131))
    # forward <8, true>; K-split cost 48 on one XCD of the pair
    f, b = _lstm_modes(("fwd_xcd8_q4", dict(wg_per_xcd=48)), "fwd_agent", ("bwd_ksplit", dict(wg_per_xcd=48, crossing_edges=0)),
                       ("bwd_unit", dict(top_tiles=2)))
    C += _both("u256_256", 11, (256, 256), 5, f, b, (1140, 141))
    # c4's arrangement: 80 forward workgroups per XCD; K-split cost 80 > 64 and unit-partitioned cost 40 > 28, so edges cross
    f, b = _lstm_modes(("fwd_xcd8_q4", dict(wg_per_xcd=80)), "fwd_agent", ("bwd_ksplit", dict(crossing_edges=(1, 9))),
                       ("bwd_unit", dict(crossing_edges=(1, 9), top_tiles=2)))
    C += _both("u256x3", 17, (256, 256, 256), 6, f, b, (5150, 4151))
    # 256 wide but not q4: the generic <8> kernel with a 256-deep K
    f, b = _lstm_modes(("fwd_xcd8", dict(wg_per_xcd=32)), "fwd_agent", "bwd_ksplit", "bwd_unit")
    C += _both("u256_128", 9, (256, 128), 4, f, b, (160, 2161))
    # two stacks in one call, different T and different len vectors
    f, b = _lstm_modes(("fwd_xcd8", dict(stacks=2)), ("fwd_agent", dict(stacks=2)), ("bwd_ksplit", dict(stacks=2)), ("bwd_unit", dict(stacks=2)))
    for r in (0, 1):
        C.append(Case("two_T/%s" % ("rv" if r else "fw"), 9, (Stack((16, 16), 5, reverse=r), Stack((32, 16), 9, reverse=r, lens="alt", cell_id_base=11)),
                      f, b, 170 + r))
    # the directions of a bidirectional encoder: 50 + 50 workgroups = the side-by-side form; tops share one [B][T+2][32] memory and read
    # their gradient from one [B][T+2][32] buffer.  BPTT: 65 K-split (33 unit-partitioned) slots per stack do not fit one launch together
    bi = (Stack((256, 256, 16), 6, reverse=0, share=(0, 32, 0)), Stack((256, 256, 16), 6, reverse=1, share=(0, 32, 16), cell_id_base=11))
    f, b = _lstm_modes(("fwd_parts", dict(stacks=2, wg_per_xcd=50, rows_per_group=16)), ("fwd_agent", dict(stacks=2)),
                       [("bwd_ksplit", dict(stacks=1, crossing_edges=(1, 9)))] * 2, [("bwd_unit", dict(stacks=1, crossing_edges=(1, 9)))] * 2)
    C.append(Case("bidi_b17", 17, bi, f, b, 4180))
    # the same at B = 70: side by side is refused (B > 64), one launch per stack
    f, b = _lstm_modes([("fwd_xcd16", dict(stacks=1, wg_per_xcd=50, launches=1))] * 2, [("fwd_agent", dict(stacks=1))] * 2,
                       [("bwd_ksplit", dict(stacks=1, launches=2))] * 2, [("bwd_unit", dict(stacks=1, launches=2))] * 2)
    C.append(Case("bidi_b70", 70, tuple(dataclasses.replace(s, lens="short") for s in bi), f, b, 172190))
    # len == NULL; a shared output buffer with columns on either side of the block (ld_out 40, out_col 4) and its gradient twin
    f, b = _lstm_modes("fwd_xcd8", "fwd_agent", "bwd_ksplit", "bwd_unit")
    C += _both("len_null", 19, (32, 48, 32), 8, f, b, (2200, 1201), lens="null", share=(0, 40, 4))
    # T = 1
    f, b = _lstm_modes("fwd_xcd8_q4", "fwd_agent", "bwd_ksplit", "bwd_unit")
    C += _both("T1", 11, (256, 256), 1, f, b, (210, 211), clips=False)
    # dh_final / dc_final NULL
    f, b = _lstm_modes("fwd_xcd8", "fwd_agent", "bwd_ksplit", "bwd_unit")
    C += _both("no_finals", 19, (32, 48, 32), 7, f, b, (220, 1221), finals=False)
    # dropout 0.8 / 0.9 / 0.7 with hs_seq and xt_seq and a consumer mask of width H on top
    f, b = _lstm_modes("fwd_xcd8", "fwd_agent", "bwd_ksplit", "bwd_unit")
    C += _both("drop_b19", 19, (32, 48, 32), 8, f, b, (230, 231), drop=Drop())
    f, b = _lstm_modes("fwd_xcd8_q4", "fwd_agent", ("bwd_ksplit", dict(crossing_edges=(1, 9))), ("bwd_unit", dict(crossing_edges=(1, 9))))
    C += _both("drop_u256x3", 17, (256, 256, 256), 6, f, b, (3240, 1241), drop=Drop(seed=99))
    # forms that never go persistent
    f, b = {m: PS for m in (0, 1, 3, 6)}, {m: PS for m in (0, 1, 3, 6)}
    C += _both("gru", 5, (12, 20), 6, f, b, (250, 251), cell="gru", modes=(0, 3))
    C += _both("residual", 5, (16, 16), 6, f, b, (260, 261), residual=(1,), modes=(0, 3))
    return C


CASES = _table()
SMALL_SCRATCH = 1000        # floats: below the first K-split slab of any case


def lens_of(case, si):
    """The len vector of stack si (None: len == NULL)."""
    st = case.stacks[si]
    if st.lens == "null":
        return None
    rng = np.random.default_rng(case.seed * 7 + si + (50 if st.lens == "alt" else 0))
    lens = rng.integers(0, (2 if st.lens == "short" else st.T) + 1, size=case.B).astype(np.int32)
    slots = rng.permutation(case.B)[:3]
    lens[slots[0]], lens[slots[1]], lens[slots[2]] = st.T, 1, 0
    return lens


def in_dims(st):
    return [F_IN] + list(st.units[:-1])


def make_inputs(case):
    """Per stack: kernels N(0,1) * 1.5 / sqrt(in + H) and biases N(0, 0.1) in engine layout (fp32), the hoisted product of layer 0 (fp64
    product rounded once to fp32), the len vector and the probes."""
    out = []
    for si, st in enumerate(case.stacks):
        rng = np.random.default_rng(case.seed * 1000 + si)
        B, T = case.B, st.T
        G = 4 if st.cell == "lstm" else 2
        d = dict(W=[], b=[], W2=[], b2=[], lens=lens_of(case, si))
        for H, i in zip(st.units, in_dims(st)):
            d["W"].append((rng.standard_normal((i + H, G * H)) * 1.5 / np.sqrt(i + H)).astype(np.float32))
            d["b"].append((rng.standard_normal(G * H) * 0.1).astype(np.float32))
            if st.cell == "gru":
                d["W2"].append((rng.standard_normal((i + H, H)) * 1.5 / np.sqrt(i + H)).astype(np.float32))
                d["b2"].append((rng.standard_normal(H) * 0.1).astype(np.float32))
        x = (rng.standard_normal((B, T, F_IN)) * (Z0_STD / 1.5) * np.sqrt((F_IN + st.units[0]) / F_IN)).astype(np.float32)
        d["x"] = x
        d["z0"] = (x.astype(np.float64) @ d["W"][0][:F_IN].astype(np.float64)).astype(np.float32)
        if st.cell == "gru":
            d["zc0"] = (x.astype(np.float64) @ d["W2"][0][:F_IN].astype(np.float64)).astype(np.float32)
        Ht = st.units[-1]
        d["R_out"] = rng.standard_normal((B, T, Ht))
        d["R_h"], d["R_c"], d["R_xt"] = rng.standard_normal((B, Ht)), rng.standard_normal((B, Ht)), rng.standard_normal((B, T, Ht))
        out.append(d)
    return out


# ---- the reference --------------------------------------------------------------------------------------------------------------------
def _t(a, dtype):
    return a.to(dtype) if isinstance(a, torch.Tensor) else torch.tensor(np.asarray(a), dtype=dtype)


def _mask(seed, stream, keep, B, T, tau, width, dtype):
    if keep >= 1.0:
        return None
    idx = ((np.arange(B) * T + tau)[:, None] * width + np.arange(width)[None, :]).astype(np.uint32)
    u = uniform01(seed, stream, idx)
    return torch.tensor((u < np.float32(keep)).astype(np.float64) / keep, dtype=dtype)


def _bf16(a):
    return a.to(torch.bfloat16).to(a.dtype)


def run_stack(st, B, d, dtype=torch.float64, mut=None, want_grad=True):
    """One stack.  d: the make_inputs record (arrays, or tensors that require grad).  mut: {name: argument} of deliberate faults
    (tests/test_rnn_check_cpu.py part d).  Returns {"layers": [records], "top": ..., "loss": tensor}; records are numpy fp64 in the
    header's layouts (sequence records [B][T][...]: no slot padding)."""
    mut = mut or {}
    T, rev, nl = st.T, st.reverse, len(st.units)
    lens = np.full(B, T, np.int64) if d["lens"] is None else np.asarray(d["lens"]).astype(np.int64)
    if "nbr_len" in mut:
        lens = lens.copy()
        lens[mut["nbr_len"]] = lens[mut["nbr_len"] + 1]
    rows = np.arange(B)
    valid_np = [t < lens for t in range(T)]
    if rev and "rev_from_T" in mut:
        tau_np = [np.full(B, T - 1 - t, np.int64) for t in range(T)]
    else:
        tau_np = [np.where(v, lens - 1 - t, 0) if rev else np.full(B, t, np.int64) for t, v in enumerate(valid_np)]
    gru = st.cell == "gru"
    fb = 0.0 if "no_forget_bias" in mut else 1.0
    dr = st.drop
    lower_x = lower_raw = None          # per processing step: the lower layer's output as this layer consumes it / as it was emitted
    layers, zs, zcs = [], [], []
    loss = torch.zeros((), dtype=dtype)
    for l, (H, i_dim) in enumerate(zip(st.units, in_dims(st))):
        W = _t(d["W"][l], dtype)
        bia = _t(d["b"][l], dtype)
        if mut.get("drop_k") == l:
            W = W.clone()
            W[i_dim + H - 1] = 0.0
        if "bf16" in mut:
            W = _bf16(W)
        if gru:
            W2, bia2 = _t(d["W2"][l], dtype), _t(d["b2"][l], dtype)
        z0 = _t(d["z0"], dtype).reshape(B, T, -1) if l == 0 else None
        zc0 = _t(d["zc0"], dtype).reshape(B, T, -1) if (l == 0 and gru) else None
        for z_in in (z0, zc0):
            if want_grad and z_in is not None and not z_in.requires_grad:
                z_in.requires_grad_(True)
        cid = st.cell_id_base + l
        h, c = torch.zeros(B, H, dtype=dtype), torch.zeros(B, H, dtype=dtype)
        rec = dict(z=[], zc=[], gates=[], cs=[], cpre=[], out=[], hs=[], xt=[], rh=[])
        for t in range(T):
            v = torch.tensor(valid_np[t])[:, None]
            tau = tau_np[t]
            if l == 0:
                zx = z0[rows, tau]
                zxc = zc0[rows, tau] if gru else None
            else:
                tx = t + 1 if ("x_next_odd" in mut and (t & 1) and t + 1 < T) else t
                xin = lower_x[tx]
                if "bf16" in mut:
                    xin = _bf16(xin)
                zx = xin @ W[:i_dim]
                zxc = xin @ W2[:i_dim] if gru else None
            hop = _bf16(h) if "bf16" in mut else h
            if gru:
                z = zx + hop @ W[i_dim:] + bia
                zz = z.view(B, H, 2)
                r, u = torch.sigmoid(zz[..., 0]), torch.sigmoid(zz[..., 1])
                rh = r * h
                zc = zxc + rh @ W2[i_dim:] + bia2
                cand = torch.tanh(zc)
                hh = u * h + (1.0 - u) * cand
                g_rec, c_new, cpre = torch.stack([r, u], -1), cand, cand
                rec["zc"].append(zc)
                rec["rh"].append(rh)
            else:
                z = zx + hop @ W[i_dim:] + bia
                zz = z.view(B, H, 4)
                gi, gj, gf, go = torch.sigmoid(zz[..., 0]), torch.tanh(zz[..., 1]), torch.sigmoid(zz[..., 2] + fb), torch.sigmoid(zz[..., 3])
                cpre = gf * c + gi * gj
                c_new = cpre if "no_clip" in mut else torch.clamp(cpre, -1.0, 1.0)
                hh = go * torch.tanh(c_new)
                g_rec = torch.stack([gi, gj, gf, go], -1)
            if want_grad:
                z.retain_grad()
                if gru:
                    zc.retain_grad()
            ho, hs = hh, hh
            if dr is not None:
                m_o = _mask(dr.seed, cid * 4 + 2, dr.keep_out, B, T, tau, H, dtype)
                m_s = _mask(dr.seed, cid * 4 + (2 if mut.get("state_mask_from_out") == l else 1), dr.keep_state, B, T, tau, H, dtype)
                ho = hh * m_o if m_o is not None else hh
                hs = hh * m_s if m_s is not None else hh
            if l in st.residual:
                ho = ho + lower_raw[t]
            xt = ho
            if dr is not None:
                if l + 1 < nl:
                    m_i = _mask(dr.seed, (cid + 1) * 4, dr.keep_in, B, T, tau, H, dtype)
                else:
                    m_i = _mask(dr.seed, dr.consumer_stream, dr.consumer_keep, B, T, tau, H, dtype)
                xt = ho * m_i if m_i is not None else ho
            zero = torch.zeros_like(ho)
            rec["z"].append(z)
            rec["gates"].append(g_rec)
            rec["cs"].append(c_new)
            rec["cpre"].append(cpre)
            rec["out"].append(torch.where(v, ho, zero))
            rec["hs"].append(torch.where(v, hs, zero))
            rec["xt"].append(torch.where(v, xt, zero))
            if "no_carry" in mut:
                h = torch.where(v, hs, zero)
                if not gru:
                    c = torch.where(v, c_new, zero)
            else:
                h = torch.where(v, hs, h)
                if not gru:
                    c = torch.where(v, c_new, c)
        rec["h_final"], rec["c_final"] = h, (None if gru else c)
        lower_x, lower_raw = rec["xt"], rec["out"]
        layers.append(rec)
    top = layers[-1]
    R_out, R_xt = _t(d["R_out"], dtype), _t(d["R_xt"], dtype)
    for t in range(T):
        loss = loss + (R_out[rows, tau_np[t]] * top["out"][t]).sum()
        if dr is not None:
            loss = loss + (R_xt[rows, tau_np[t]] * top["xt"][t]).sum()
    if st.finals:
        sel = torch.tensor(lens == T, dtype=dtype)[:, None] if "dh_at_T" in mut else 1.0
        loss = loss + (_t(d["R_h"], dtype) * top["h_final"] * sel).sum()
        if not gru:
            loss = loss + (_t(d["R_c"], dtype) * top["c_final"] * sel).sum()
    if want_grad:
        loss.backward()

    def place(steps, tail):
        a = np.zeros((B, T) + tail)
        for t, s in enumerate(steps):
            ok = valid_np[t]
            a[rows[ok], tau_np[t][ok]] = s.detach().numpy().astype(np.float64)[ok].reshape((int(ok.sum()),) + tail)
        return a

    G = 2 if gru else 4
    res = []
    for l, rec in enumerate(layers):
        H = st.units[l]
        r = dict(gates=place(rec["gates"], (H, G)), cs=place(rec["cs"], (H,)), cpre=place(rec["cpre"], (H,)), out=place(rec["out"], (H,)),
                 hs=place(rec["hs"], (H,)), xt=place(rec["xt"], (H,)), h_final=rec["h_final"].detach().numpy().astype(np.float64))
        if not gru:
            r["c_final"] = rec["c_final"].detach().numpy().astype(np.float64)
        else:
            r["rh"] = place(rec["rh"], (H,))
        if want_grad:
            zero = torch.zeros(B, G * H, dtype=dtype)
            r["dgates"] = place([z.grad if z.grad is not None else zero for z in rec["z"]], (H, G))
            if gru:
                zero = torch.zeros(B, H, dtype=dtype)
                r["dgates2"] = place([z.grad if z.grad is not None else zero for z in rec["zc"]], (H,))
        res.append(r)
    return dict(layers=res, lens=lens, loss=loss)


def reference(case, inp=None, dtype=torch.float64, mut=None):
    """Every stack of a case: [run_stack record].  mut = (stack index, {fault: argument})."""
    inp = inp or make_inputs(case)
    return [run_stack(st, case.B, inp[si], dtype, mut[1] if (mut and mut[0] == si) else None) for si, st in enumerate(case.stacks)]


QUANT = ("gates", "cs", "out", "hs", "xt", "h_final", "c_final", "rh", "dgates", "dgates2")


def noise_of(ref64, ref32):
    """Per quantity: (largest |fp32 twin - fp64| over the case, largest |fp64| entry)."""
    out = {}
    for q in QUANT:
        gap, big = 0.0, 0.0
        for s64, s32 in zip(ref64, ref32):
            for a, b in zip(s64["layers"], s32["layers"]):
                if q in a:
                    gap, big = max(gap, float(np.abs(a[q] - b[q]).max(initial=0.0))), max(big, float(np.abs(a[q]).max(initial=0.0)))
        out[q] = (gap, big)
    return out


_CACHE = {}


def fixture(case):
    """(inputs, fp64 reference, noise) of a case, computed once per process and never modified by its users."""
    if case.name not in _CACHE:
        inp = make_inputs(case)
        r64 = reference(case, inp)
        _CACHE[case.name] = (inp, r64, noise_of(r64, reference(case, inp, torch.float32)))
    return _CACHE[case.name]


def conditions(case, ref, noise):
    """What tests/test_rnn_check_cpu.py part (b) asks of a case, measured on the reference alone: the distance of the nearest pre-clip
    cell state from +-1, the share of clipped cell states at t < len, the share of recorded gate values beyond 0.95 or below 0.05 (all
    recorded gates, as the records hold them) and the same over the sigmoid gates alone, and the largest relative noise."""
    near, tot, clip, ng, sat, ns, sat_s = 1.0, 0, 0, 0, 0, 0, 0
    for si, s in enumerate(ref):
        live = np.arange(case.stacks[si].T)[None, :] < s["lens"][:, None]
        lstm = case.stacks[si].cell == "lstm"
        for r in s["layers"]:
            g = r["gates"][live]
            ng, sat = ng + g.size, sat + int(((g > 0.95) | (g < 0.05)).sum())
            gs = g[..., [0, 2, 3]] if lstm else g
            ns, sat_s = ns + gs.size, sat_s + int(((gs > 0.95) | (gs < 0.05)).sum())
            if lstm:
                cp = r["cpre"][live]
                tot, clip = tot + cp.size, clip + int((np.abs(cp) >= 1.0).sum())
                near = min(near, float(np.abs(np.abs(cp) - 1.0).min(initial=1.0)))
    rel = max(v[0] / v[1] for v in noise.values() if v[1] > 0)
    return dict(near=near, clipped=clip / max(tot, 1), saturated=sat / max(ng, 1), saturated_sigmoid=sat_s / max(ns, 1), noise_rel=rel)


def tolerance(q, noise, ref_max=0.0):
    """max(T_suite, 8 x noise): the rule of tests/test_gpu_regime.py."""
    t = T_SUITE_DGATES * max(1.0, ref_max) if q.startswith("dgates") else T_SUITE
    return max(t, 8.0 * noise[q][0])


# ---- the engine's buffers -------------------------------------------------------------------------------------------------------------
def layout(case):
    """Every buffer a call on this case owns, as {key: spec}: key = (stack, layer, name) or ("shared", id, "out" / "dout"); spec =
    dict(n floats, kind).  Sizes are exactly the header's."""
    L = {}
    B = case.B
    for si, st in enumerate(case.stacks):
        T, nl, gru = st.T, len(st.units), st.cell == "gru"
        G = 2 if gru else 4
        for l, H in enumerate(st.units):
            res = l in st.residual
            k = lambda name: (si, l, name)
            L[k("gates")] = B * T * H * G
            L[k("cs")] = B * T * H
            L[k("dgates")] = B * T * H * G
            L[k("h_final")] = B * H
            L[k("state")] = (6 if (st.drop or res) else 4) * B * H
            L[k("dstate")] = (14 if res else 12) * B * H
            if not gru:
                L[k("c_final")] = B * H
            else:
                L[k("rh")] = B * T * H
                L[k("dgates2")] = B * T * H
            if st.drop or res:
                L[k("hs")] = B * (T + 2) * H
            if st.drop:
                L[k("xt")] = B * (T + 2) * H
            top = l == nl - 1
            if top and st.share:
                L[("shared", st.share[0], "out")] = B * (T + 2) * st.share[1]
                L[("shared", st.share[0], "dout")] = B * (T + 2) * st.share[1]
            else:
                L[k("out")] = B * (T + 2) * H
                if top:
                    L[k("dout")] = B * (T + 2) * H
    return L


def out_place(case, si, l):
    """(buffer key, ld_out, out_col) of a layer's output; the top layer's dout has the same placement under name "dout"."""
    st = case.stacks[si]
    if l == len(st.units) - 1 and st.share:
        return ("shared", st.share[0], "out"), st.share[1], st.share[2]
    return (si, l, "out"), st.units[l], 0


def alloc(n):
    a = np.empty(n + 2 * GUARD, np.float32)
    a.view(np.uint32)[:] = PATTERN
    return a


def inner(a):
    return a[GUARD:len(a) - GUARD]


def initial_buffers(case, inp, ref):
    """The buffers as the caller hands them to avsr_rnn_fwd, each inside its NaN band: everything the call must write is NaN pattern,
    slots 0 and T+1 of the slot-padded sequences are zero (the caller's part of the contract), `gates` (and a GRU's `cs`) of layer 0
    hold the hoisted product, dout holds the probe, columns of a shared buffer outside every block hold a finite pattern."""
    bufs = {k: alloc(n) for k, n in layout(case).items()}
    B = case.B
    for si, st in enumerate(case.stacks):
        T, nl = st.T, len(st.units)
        inner(bufs[(si, 0, "gates")])[:] = inp[si]["z0"].reshape(-1)
        if st.cell == "gru":
            inner(bufs[(si, 0, "cs")])[:] = inp[si]["zc0"].reshape(-1)
        for l, H in enumerate(st.units):
            key, ld, col = out_place(case, si, l)
            o = inner(bufs[key]).reshape(B, T + 2, ld)
            o[:, 0, col:col + H] = 0.0
            o[:, T + 1, col:col + H] = 0.0
            for name in ("hs", "xt"):
                if (si, l, name) in bufs:
                    s = inner(bufs[(si, l, name)]).reshape(B, T + 2, H)
                    s[:, 0] = 0.0
                    s[:, T + 1] = 0.0
        # the probe: gradient wrt `out` (with dropout, the consumer's gradient wrt xt_seq comes back through its mask)
        key, ld, col = out_place(case, si, nl - 1)
        H = st.units[-1]
        dk = key[:2] + ("dout",)
        do = inner(bufs[dk]).reshape(B, T + 2, ld)
        g = np.array(inp[si]["R_out"], np.float64)
        if st.drop:
            idx = np.arange(B * T * H, dtype=np.uint32).reshape(B, T, H)
            m = (uniform01(st.drop.seed, st.drop.consumer_stream, idx) < np.float32(st.drop.consumer_keep)) / st.drop.consumer_keep
            g = g + inp[si]["R_xt"] * m
        do[:, 0, col:col + H] = 0.0
        do[:, T + 1, col:col + H] = 0.0
        do[:, 1:T + 1, col:col + H] = g
    # columns of a shared buffer that belong to no block: a finite pattern that must come back bit-unchanged
    for key, a in bufs.items():
        if key[0] != "shared":
            continue
        owners = [(st.share[2], st.units[-1]) for st in case.stacks if st.share and st.share[0] == key[1]]
        ld = [st.share[1] for st in case.stacks if st.share and st.share[0] == key[1]][0]
        o = inner(a).reshape(case.B, -1, ld)
        for c in range(ld):
            if not any(c0 <= c < c0 + w for c0, w in owners):
                o[:, :, c] = 0.25 + c
    return bufs


def expected_buffers(case, inp, ref):
    """The buffers as a correct engine leaves them after avsr_rnn_fwd + avsr_rnn_bwd, built from the reference (the CPU side of the
    checker's tests mutates copies of these).  Entries the engine need not write (records at t >= len, scratch) keep their fill."""
    bufs = initial_buffers(case, inp, ref)
    B = case.B
    for si, st in enumerate(case.stacks):
        T = st.T
        lens = ref[si]["lens"]
        live = (np.arange(T)[None, :] < lens[:, None])
        for l, H in enumerate(st.units):
            r = ref[si]["layers"][l]
            G = r["gates"].shape[-1]
            for name, tail in (("gates", (H, G)), ("cs", (H,)), ("rh", (H,))):
                if (si, l, name) in bufs:
                    a = inner(bufs[(si, l, name)]).reshape((B, T) + tail)
                    a[live] = r[name][live]
            for name in ("dgates", "dgates2"):
                if (si, l, name) in bufs:
                    inner(bufs[(si, l, name)])[:] = r[name].reshape(-1)
            inner(bufs[(si, l, "h_final")])[:] = r["h_final"].reshape(-1)
            if "c_final" in r:
                inner(bufs[(si, l, "c_final")])[:] = r["c_final"].reshape(-1)
            key, ld, col = out_place(case, si, l)
            inner(bufs[key]).reshape(B, T + 2, ld)[:, 1:T + 1, col:col + H] = r["out"]
            for name in ("hs", "xt"):
                if (si, l, name) in bufs:
                    inner(bufs[(si, l, name)]).reshape(B, T + 2, H)[:, 1:T + 1] = r[name]
    return bufs


# ---- the checker ----------------------------------------------------------------------------------------------------------------------
def _first(bad):
    idx = np.argwhere(bad)
    return tuple(int(i) for i in idx[0]) if len(idx) else None


def check(case, inp, ref, noise, before, after, again=None, err_word=0, log=None):
    """Judge the engine's buffers `after` a forward + BPTT on `before` (initial_buffers) against the reference.  Returns None, or the
    first offence as (stack, layer, quantity, b, t, u, what).  again: the buffers of a second identical call (bit-equal or an offence).
    log: a list that receives (quantity, largest error, bound) per compared quantity."""
    B = case.B
    if err_word != 0:
        return (-1, -1, "sync", -1, -1, -1, "sticky error word %d" % err_word)
    for key in before:                                  # the NaN band around every buffer
        for part, sl in (("low", slice(0, GUARD)), ("high", slice(-GUARD, None))):
            if not (after[key].view(np.uint32)[sl] == PATTERN).all():
                i = _first(after[key].view(np.uint32)[sl] != PATTERN)[0]
                return (key[0], key[1], key[2], -1, -1, -1, "wrote %s guard band at word %d" % (part, i))
    worst = {}

    def cmp(si, l, q, got, want, mask, scale_max=0.0):
        tol = tolerance(q, noise, scale_max)
        gap = np.where(mask, np.abs(got.astype(np.float64) - want), 0.0)
        gap = np.where(mask & ~np.isfinite(got), np.inf, gap)
        worst[q] = max(worst.get(q, 0.0), float(gap.max(initial=0.0)))
        if log is not None:
            log.append((si, l, q, float(gap.max(initial=0.0)), tol))
        f = _first(gap > tol)
        if f is None:
            return None
        b, t, u = (f + (-1, -1))[:3] if got.ndim >= 3 else (f[0], -1, f[1])
        return (si, l, q, b, t, u, "got %r want %r (bound %.3g)" % (float(got[f]), float(want[f]), tol))

    for si, st in enumerate(case.stacks):
        T = st.T
        lens = ref[si]["lens"]
        live = (np.arange(T)[None, :] < lens[:, None])
        for l, H in enumerate(st.units):
            r = ref[si]["layers"][l]
            G = r["gates"].shape[-1]
            m3, m4 = np.broadcast_to(live[:, :, None], (B, T, H)), np.broadcast_to(live[:, :, None, None], (B, T, H, G))
            # records at t < len
            for q, tail, m in (("gates", (H, G), m4), ("cs", (H,), m3), ("rh", (H,), m3)):
                if (si, l, q) in after:
                    bad = cmp(si, l, q, inner(after[(si, l, q)]).reshape((B, T) + tail), r[q], m)
                    if bad:
                        return bad
            # outputs: tolerance at t < len, exact zeros at len <= t < T and in slots 0 and T+1, other columns bit-unchanged
            key, ld, col = out_place(case, si, l)
            o = inner(after[key]).reshape(B, T + 2, ld)
            o0 = inner(before[key]).reshape(B, T + 2, ld)
            seqs = [("out", o[:, :, col:col + H])] + [(q, inner(after[(si, l, q)]).reshape(B, T + 2, H)) for q in ("hs", "xt") if (si, l, q) in after]
            for q, s in seqs:
                bad = cmp(si, l, q, s[:, 1:T + 1], r[q], m3)
                if bad:
                    return bad
                pad = s.view(np.uint32)[:, 1:T + 1] & np.uint32(0x7FFFFFFF)
                f = _first((pad != 0) & ~m3)
                if f:
                    return (si, l, q, f[0], f[1], f[2], "not zero at t >= len: %r" % float(s[f[0], f[1] + 1, f[2]]))
                for slot in (0, T + 1):
                    f = _first((s.view(np.uint32)[:, slot] & np.uint32(0x7FFFFFFF)) != 0)
                    if f:
                        return (si, l, q, f[0], slot - 1, f[1], "guard slot %d not zero: %r" % (slot, float(s[f[0], slot, f[1]])))
            if key[0] == "shared":
                own = np.zeros(ld, bool)
                for s2 in case.stacks:
                    if s2.share and s2.share[0] == key[1]:
                        own[s2.share[2]:s2.share[2] + s2.units[-1]] = True
                f = _first((o.view(np.uint32) != o0.view(np.uint32))[:, :, ~own])
                if f:
                    return (si, l, "out", f[0], f[1] - 1, int(np.flatnonzero(~own)[f[2]]), "column outside every block changed")
            # final states
            for q in ("h_final", "c_final"):
                if q in r:
                    bad = cmp(si, l, q, inner(after[(si, l, q)]).reshape(B, H), r[q], np.ones((B, H), bool))
                    if bad:
                        return bad
            # dgates at every t, exact zeros at t >= len
            for q, tail, m in (("dgates", (H, G), m4), ("dgates2", (H,), m3)):
                if q in r:
                    got = inner(after[(si, l, q)]).reshape((B, T) + tail)
                    bad = cmp(si, l, q, got, r[q], np.ones_like(m), float(np.abs(r[q]).max(initial=0.0)))
                    if bad:
                        return bad
                    f = _first(((got.view(np.uint32) & np.uint32(0x7FFFFFFF)) != 0) & ~m)
                    if f:
                        return (si, l, q, f[0], f[1], f[2], "not zero at t >= len: %r" % float(got[f]))
            # dout is an input: bit-unchanged
            if l == len(st.units) - 1:
                dk = key[:2] + ("dout",)
                if not (after[dk].view(np.uint32) == before[dk].view(np.uint32)).all():
                    return (si, l, "dout", -1, -1, -1, "the call wrote its input gradient")
    if again is not None:
        for key in after:
            if key[2] in ("state", "dstate"):
                continue
            d = after[key].view(np.uint32) != again[key].view(np.uint32)
            if d.any():
                return (key[0], key[1], key[2], -1, -1, -1, "second identical call differs at word %d" % (_first(d)[0] - GUARD))
    return None


# ---- descriptors ----------------------------------------------------------------------------------------------------------------------
def descriptors(case, addr):
    """The RnnStack descriptors of a case.  addr(key) -> address of the first float of that buffer (past its guard band), or of
    ("w" / "wt" / "bias" / "w2" / "wt2" / "bias2", stack, layer), ("len" / "dh_final" / "dc_final" / "seed", stack)."""
    from avsr_tf1_amd._lib import RnnStack
    out = []
    for si, st in enumerate(case.stacks):
        S = RnnStack()
        S.B, S.T, S.reverse, S.n_layers, S.cell = case.B, st.T, st.reverse, len(st.units), int(st.cell == "gru")
        S.len = None if st.lens == "null" else addr(("len", si))
        if st.finals:
            S.dh_final = addr(("dh_final", si))
            if st.cell == "lstm":
                S.dc_final = addr(("dc_final", si))
        if st.drop:
            dr = st.drop
            S.seed = addr(("seed", si))
            S.keep_in, S.keep_state, S.keep_out, S.consumer_keep = dr.keep_in, dr.keep_state, dr.keep_out, dr.consumer_keep
            S.consumer_stream, S.consumer_width = dr.consumer_stream, st.units[-1]
        S.cell_id_base = st.cell_id_base
        for l, (H, i_dim) in enumerate(zip(st.units, in_dims(st))):
            Ly = S.layer[l]
            key, ld, col = out_place(case, si, l)
            Ly.units, Ly.in_dim, Ly.hoisted, Ly.out_col = H, i_dim, int(l == 0), col
            Ly.wt, Ly.w, Ly.bias = addr(("wt", si, l)), addr(("w", si, l)), addr(("bias", si, l))
            Ly.gates, Ly.cs, Ly.out, Ly.ld_out = addr((si, l, "gates")), addr((si, l, "cs")), addr(key), ld
            Ly.state, Ly.h_final = addr((si, l, "state")), addr((si, l, "h_final"))
            Ly.dgates, Ly.dstate = addr((si, l, "dgates")), addr((si, l, "dstate"))
            Ly.residual = int(l in st.residual)
            if st.cell == "lstm":
                Ly.c_final = addr((si, l, "c_final"))
            else:
                Ly.wt2, Ly.w2, Ly.bias2 = addr(("wt2", si, l)), addr(("w2", si, l)), addr(("bias2", si, l))
                Ly.rh_seq, Ly.dgates2 = addr((si, l, "rh")), addr((si, l, "dgates2"))
            if st.drop or Ly.residual:
                Ly.hs_seq = addr((si, l, "hs"))
            if st.drop:
                Ly.xt_seq = addr((si, l, "xt"))
            if l == len(st.units) - 1:
                Ly.dout, Ly.ld_dout, Ly.dout_col = addr(key[:2] + ("dout",)), ld, col
        out.append(S)
    return out


def plan(case, bwd, mode, scratch_floats=64 << 20):
    """ops.rnn_plan of a case (no GPU: every pointer is one dummy address)."""
    from avsr_tf1_amd import ops
    return ops.rnn_plan(descriptors(case, lambda key: 64), bwd=bwd, mode=max(mode, 1), sync_ints=(1 << 20) if mode else 0, scratch_floats=scratch_floats)


def plan_matches(recs, want):
    """Does a plan (list of records) say what a row of the table names?  want: form | (form, {field: value or (lo, hi)}) | [those]."""
    want = want if isinstance(want, list) else [want]
    if len(recs) != len(want):
        return False
    for r, w in zip(recs, want):
        form, fields = (w, {}) if isinstance(w, str) else w
        if r["form"] != form:
            return False
        for k, v in fields.items():
            if not (v[0] <= r[k] <= v[1] if isinstance(v, tuple) else r[k] == v):
                return False
    return True
