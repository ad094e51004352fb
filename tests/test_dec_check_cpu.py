"""Judge the judge of the attention-decoder conformance suite, on the CPU (tests/ref_dec.py; the GPU side is
tests/test_gpu_dec_conformance.py).

(a) the reference agrees to 1e-10 with the oracle's own formulation of the block: oracle._Cell, _Mechanism, attention_wrapper_step, the
    helper logic of forward_train / greedy_decode, and autograd;
(b) the conditions on the inputs hold for every row, no element excluded: noise below the cap, every greedy argmax ahead of the runner-up
    and every sampling uniform away from the edges of its CDF bin by 100 x the case's own logits bound max(T_suite, 8 x noise), every
    select draw 1e-3 from sampling_prob;
(c) the checker accepts the reference's own buffers and rejects every fault of the list, each applied to a copy of them;
(d) the plan comparison is unit-tested on hand-made records;
(e) avsr_attn_rnn_plan, which needs no GPU, answers every row of the table under every avsr_attn_rnn_set_fused setting."""
import numpy as np
import pytest
import torch

import ref_dec as R
from oracle import avsr_oracle as O


# ---- (a) the reference against the oracle's formulation ---------------------------------------------------------------------------------
def _oracle_block(case, key, inp):
    """The block through oracle._Cell / _Mechanism / attention_wrapper_step with the loop logic of forward_train (mode 2, mode 0) or
    greedy_decode (mode 1), in the ORACLE's layouts (gate columns blocked i | j | f | o), fp64, with autograd of the same probe."""
    mode, V = key
    B, L, H, E = case.B, case.L, case.H, case.E
    nm = len(case.mems)
    A = nm * H
    t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    perm = np.array([4 * u + g for g in range(4) for u in range(H)])          # oracle column g*H + u = engine column 4*u + g
    Wo = inp["W"][:, perm].astype(np.float64)
    if mode == 0:         # the hoisted product is the cell's input: identity rows in place of the kernel's input rows
        Wo = np.concatenate([np.eye(4 * H), Wo[E:]], 0)
    P = {"c/kernel": t64(Wo).requires_grad_(True), "c/bias": t64(inp["bias"][perm]).requires_grad_(True)}
    cell = O._Cell(P, "c", "lstm", H)
    if case.drop and mode != 1:
        cell.set_dropout(case.drop, R.CELL_ID, L, inp["seed"])
    mechs = []
    for M, m in zip(case.mems, inp["mem"]):
        X = O._Mechanism.__new__(O._Mechanism)
        X.type = M.type
        X.mask = torch.arange(M.T)[None, :] < torch.tensor(m["len"].astype(np.int64))[:, None]
        X.values = t64(m["values"]) * X.mask[:, :, None]
        X.keys = t64(m["keys"]).requires_grad_(True)
        X.layer = t64(m["watt"]).requires_grad_(True)
        X.g = t64(m["g"][0]) if "g" in m else None
        if "v" in m:
            X.Wq, X.v = t64(m["wq"]).requires_grad_(True), t64(m["v"])
            X.b = t64(m["bq"]) if "bq" in m else None
            if M.type == "normed_bahdanau":
                X.g = torch.sqrt(torch.sum(X.v * X.v))                         # the engine is handed g * v / |v|: g = |v| leaves v as it is
        mechs.append(X)
    h0 = t64(inp["h0"] if case.h0 else np.zeros((B, H))).requires_grad_(True)
    c0 = t64(inp["c0"] if case.h0 else np.zeros((B, H))).requires_grad_(True)
    state, att = (c0, h0), torch.zeros(B, A, dtype=torch.float64)
    out = dict(cell_out=[], att=[], logits=[])
    steplen = torch.tensor(inp["steplen"].astype(np.int64))
    if mode == 0:
        x_all = t64(inp["zx"]).reshape(B, L, 4 * H)[:, :, perm]
    else:
        emb, wout, bout = t64(inp["emb"]), t64(inp["wout"]), t64(inp["bout"])
    fed = np.zeros((B, L), np.int64)
    fed[:, 0] = R.GO
    tok, ids = np.full(B, R.GO, np.int64), np.zeros((B, L), np.int64)
    finished = np.zeros(B, bool)
    for l in range(L):
        x = x_all[:, l] if mode == 0 else emb[torch.tensor(fed[:, l] if mode == 2 else tok)]
        o, ns, natt, _ = O.attention_wrapper_step(cell, mechs, bool(case.oa), x, state, att, l)
        fin = torch.tensor(finished)[:, None] if mode == 1 else (l >= steplen)[:, None]
        co = ns[1] if not cell.drop else None
        if mode >= 1:
            lg = o @ wout + bout
            lg = torch.where(fin, torch.zeros_like(lg), lg)
            out["logits"].append(lg)
            if mode == 2 and l + 1 < L:
                fed[:, l + 1] = inp["labels"][:, l]
                if case.prob > 0:
                    idx = (np.arange(B) * L + l).astype(np.uint32)
                    sel = O.uniform01(inp["seed"], O.STREAM_SS_SELECT, idx) < np.float32(case.prob)
                    us = O.uniform01(inp["seed"], O.STREAM_SS_SAMPLE, idx)
                    for b in range(B):
                        if sel[b]:
                            fed[b, l + 1] = O.categorical_f32(lg.detach().numpy()[b], us[b])
            if mode == 1:
                best = lg.detach().numpy().argmax(axis=1)
                ids[:, l] = np.where(finished, 0, best)
                tok = np.where(finished, tok, best)
                finished = finished | (best == R.EOS)
        out["att"].append(torch.where(fin, torch.zeros_like(natt), natt))
        out["cell_out"].append(co)
        state = O._map_state(lambda n, s: torch.where(fin, s, n), ns, state)
        att = torch.where(fin, att, natt)
    res = dict(att=torch.stack(out["att"], 1), h=state[1], c=state[0], fed=fed, ids=ids)
    if mode >= 1:
        res["logits"] = torch.stack(out["logits"], 1)
    if not cell.drop:
        res["cell_out"] = torch.stack(out["cell_out"], 1)
    if mode != 1:
        loss = (t64(inp["datt_ext"]) * res["att"]).sum()
        if not cell.drop:                       # with dropout the emitted (output-masked) cell output is not exposed by the oracle's step
            live = (torch.arange(L)[None, :] < steplen[:, None])[:, :, None]
            loss = loss + (t64(inp["dcell_ext"]) * torch.where(live, res["cell_out"], torch.zeros_like(res["cell_out"]))).sum()
        if case.finals:
            loss = loss + (t64(inp["dh_final"]) * res["h"]).sum() + (t64(inp["dc_final"]) * res["c"]).sum()
        loss.backward()
        res.update(dbias=P["c/bias"].grad, dh0=h0.grad, dc0=c0.grad, dkeys=[X.keys.grad for X in mechs], dwatt=[X.layer.grad for X in mechs],
                   dwq=[getattr(X, "Wq", None) is not None and X.Wq.grad for X in mechs], perm=perm)
    return res


ORACLE_KEYS = [("no_finals_no_h0", (0, 0)), ("attentive_129", (0, 0)), ("two_mode0_v1", (0, 0)), ("two_v2", (2, 28)), ("two_v2", (1, 41)),
               ("scaled_D_ne_H_drop", (2, 32)), ("v33", (1, 33)), ("bahdanau", (2, 28)), ("bahdanau", (1, 28)), ("normed_bahdanau", (2, 41)),
               ("normed_bahdanau", (1, 28)), ("min_empty_quarter", (2, 28))]


@pytest.mark.parametrize("name,key", ORACLE_KEYS, ids=["%s-mode%d-V%d" % (n, k[0], k[1]) for n, k in ORACLE_KEYS])
def test_reference_agrees_with_the_oracle(name, key):
    case = R.BY_NAME[name]
    mode, V = key
    inp, ref, _ = R.fixture(case, key)
    if case.drop and mode != 1:
        # the oracle's probe cannot see the emitted cell output under dropout: the reference is rerun with that probe switched off
        # and slot 0 of xs, which the caller rounds to fp32 after its own dropout, is given unrounded as the oracle forms it
        inp = dict(inp, dcell_ext=np.zeros_like(inp["dcell_ext"]))
        if mode == 2:
            keep = case.drop[0]
            inp["xs0"] = np.where(inp["xs0"] != 0, inp["emb"][R.GO].astype(np.float64)[None] / keep, 0.0)
        ref = R.run(case, key, inp)
    orc = _oracle_block(case, key, inp)
    B, L, H = case.B, case.L, case.H
    live = ref["live"]
    near = lambda a, b, what: np.testing.assert_allclose(np.asarray(a), b.detach().numpy() if isinstance(b, torch.Tensor) else b,
                                                          rtol=0, atol=1e-10, err_msg=what)
    if mode == 1:
        assert (ref["ids"] == orc["ids"]).all()
        assert (ref["steplen"] < L).any() or B * L < 20
    near(ref["att"][:, 1:] * live[:, :, None], orc["att"] * torch.tensor(live)[:, :, None], "att")
    if "cell_out" in orc:
        near(ref["cell_out"][:, 1:][live], orc["cell_out"].detach().numpy()[live], "cell_out")
    if mode >= 1:
        near(ref["logits"], orc["logits"], "logits")
    if mode == 2:
        assert (ref["fed"] == orc["fed"]).all()
    if mode != 1:
        near(ref["h_final"], orc["h"], "h_final"), near(ref["c_final"], orc["c"], "c_final")
        near(ref["dgates"].reshape(B * L, 4 * H).sum(0)[orc["perm"]], orc["dbias"], "dgates (through the bias gradient)")
        near(ref["dh0"], orc["dh0"], "dh0"), near(ref["dc0"], orc["dc0"], "dc0")
        q = ref["cell_out"][:, 1:]
        for mi, (M, m) in enumerate(zip(case.mems, inp["mem"])):
            r = ref["mem"][mi]
            op = np.concatenate([q, r["ctx"]], -1)
            near(np.einsum("blk,blh->kh", op, ref["datt"][:, :, mi * H:(mi + 1) * H]), orc["dwatt"][mi], "datt / ctx (through d W_att)")
            if "dpq" in r:
                near(np.einsum("blk,blh->kh", q, r["dpq"]), orc["dwq"][mi], "dpq (through d W_q)")
            else:
                g = float(m["g"][0]) if "g" in m else 1.0
                near(np.einsum("blt,blh->bth", r["dscores"], q) * g, orc["dkeys"][mi], "dscores (through d keys)")


# ---- (b) the conditions on the inputs ---------------------------------------------------------------------------------------------------
ALL_KEYS = [(c.name, k) for c in R.CASES for k in c.keys()]


@pytest.mark.parametrize("name,key", ALL_KEYS, ids=["%s-mode%d-V%d" % (n, k[0], k[1]) for n, k in ALL_KEYS])
def test_conditions_hold(name, key):
    case = R.BY_NAME[name]
    inp, ref, noise = R.fixture(case, key)
    cond = R.conditions(case, key, ref, noise)
    assert cond["noise_rel"] < R.NOISE_CAP, cond
    need = R.margin_of(noise)                # 100 x this case's own logits bound max(T_suite, 8 x noise)
    assert need >= R.MARGIN_FACTOR * R.T_SUITE and (key[0] == 0 or need == R.MARGIN_FACTOR * R.tolerance("logits", noise))
    assert cond["margin"] >= need and cond["edge"] >= need and cond["bern"] >= R.BERN_MARGIN, (cond, need)
    assert R.holds(case, key, inp, ref, noise), (cond, need)
    # the len vectors hold T, 1, a full quarter and a quarter plus one; steplen holds L, 1 and a value between (where B allows)
    wpr = 32 // (case.plan[key[0]]["rows"] if case.plan[key[0]] else 8)
    for M, m in zip(case.mems, inp["mem"]):
        ch = (M.T + wpr - 1) // wpr
        want = [M.T, 1, ch, min(ch + 1, M.T)][:case.B]
        assert all(min(max(v, 1), M.T) in m["len"] for v in want), (m["len"], want)
    if key[0] != 1:
        assert all(v in inp["steplen"] for v in [case.L, 1, max((case.L + 1) // 2, 1)][:case.B]), inp["steplen"]


# ---- (c) the checker rejects the faults -------------------------------------------------------------------------------------------------
def _bufs(case, key, mut=None):
    inp, ref, noise = R.fixture(case, key)
    before = R.initial_buffers(case, key, inp)
    bad = R.run(case, key, inp, mut=mut) if mut else ref
    return inp, ref, noise, before, R.expected_buffers(case, key, inp, bad)


# fault -> (row, (mode, V), {mutation of the reference})
REF_FAULTS = {
    "softmax_over_T": ("two_v2", (2, 28), {"softmax_over_T": 1}),
    "neighbour_len": ("scaled_D_ne_H_drop", (2, 32), {"nbr_len": 0}),
    "short_quarter_dropped": ("min_empty_quarter", (2, 28), {"drop_quarter": 1}),
    "empty_quarter_zero_max": ("min_empty_quarter", (2, 28), {"empty_zero_max": 1}),
    "contexts_swapped_in_att": ("dec_b67", (2, 28), {"ctx_swap": 1}),
    "scaled_luong_g_missing": ("scaled_D_ne_H_drop", (2, 32), {"no_g": 1}),
    "normed_bahdanau_bias_missing": ("normed_bahdanau", (2, 28), {"no_bq": 1}),
    "undropped_attention_fed_back": ("scaled_D_ne_H_drop", (2, 32), {"undropped_att_fed": 1}),
    "state_mask_from_output_stream": ("attentive_r16", (0, 0), {"state_mask_from_out": 1}),
    "state_not_carried": ("two_v2", (0, 0), {"no_carry": 1}),
    "logits_not_zero_past_steplen": ("two_v2", (2, 41), {"logits_past_steplen": 1}),
    "sample_index_off_by_one": ("two_v2", (2, 28), {"sample_idx_off": 1}),
    "h0_enters_at_step_1": ("attentive_r16", (0, 0), {"h0_at_step1": 1}),
    "dh_final_at_L": ("attentive_r16", (0, 0), {"dh_at_L": 1}),
    "operands_bf16": ("wide_cpw7", (2, 28), {"bf16": 1}),
    "operands_bf16_greedy": ("bahdanau", (1, 28), {"bf16": 1}),
}


@pytest.mark.parametrize("fault", sorted(REF_FAULTS))
def test_checker_rejects_a_faulty_engine(fault):
    name, key, mut = REF_FAULTS[fault]
    case = R.BY_NAME[name]
    inp, ref, noise, before, good = _bufs(case, key)
    assert R.check(case, key, inp, ref, noise, before, good, again=good) is None
    if "nbr_len" in mut:                         # the first live row whose neighbour's memory has another length
        ln = inp["mem"][0]["len"]
        mut = {"nbr_len": int(np.flatnonzero(ln[:-1] != ln[1:])[0])}
    inp, ref, noise, before, bad = _bufs(case, key, mut)
    assert R.check(case, key, inp, ref, noise, before, bad) is not None, fault


def _swap_rows(a, shape, i, j):
    v = R.inner(a).reshape(shape)
    v[[i, j]] = v[[j, i]]


def _buffer_faults():
    """fault -> (row, (mode, V), function that damages a copy of the correct buffers in place)."""
    F = {}
    c = R.BY_NAME["two_v2"]
    B, L, H = c.B, c.L, c.H
    F["rows_b_b8_swapped"] = ("two_v2", (2, 28), lambda b: _swap_rows(b["ctx0"], (B, L, 32), 0, 8))
    F["rows_b_b8_swapped_bptt"] = ("two_v2", (2, 28), lambda b: _swap_rows(b["dgates"], (B, L, H, 4), 0, 8))

    def gates_swapped(b):
        g = R.inner(b["gates"]).reshape(B, L, H, 4)
        g[:, :, 5, [0, 2]] = g[:, :, 5, [2, 0]]
    F["two_gates_swapped"] = ("two_v2", (2, 28), gates_swapped)
    v = R.BY_NAME["v33"]

    def col32(b):
        R.inner(b["logits"]).reshape(v.B, v.L, 33)[:, :, 32] = 0.0
    F["symbol_32_dropped"] = ("v33", (2, 33), col32)

    def dctx_swapped(b):
        b["dctx0"], b["dctx1"] = b["dctx1"], b["dctx0"]
    F["dctx_swapped"] = ("dec_b67", (2, 28), dctx_swapped)
    F["float_in_guard_slot"] = ("two_v2", (2, 28), lambda b: R.inner(b["att"]).reshape(B, L + 1, 2 * H).__setitem__((3, 0, 7), 1e-30))
    F["float_in_dead_slot"] = ("two_v2", (2, 28), lambda b: R.inner(b["cell_out"]).reshape(B, L + 1, H).__setitem__((1, L, 0), 1e-30))
    F["float_in_a_band"] = ("two_v2", (2, 28), lambda b: b["cs"].__setitem__(R.GUARD - 1, 0.0))
    F["float_past_fused_ws"] = ("two_v2", (2, 28), lambda b: b["fused_ws"].__setitem__(len(b["fused_ws"]) - R.GUARD, 0.0))
    F["float_before_fused_ws"] = ("two_v2", (2, 28), lambda b: b["fused_ws"].__setitem__(R.GUARD - 1, 0.0))
    F["dead_row_written"] = ("two_v2", (2, 28), lambda b: R.inner(b["cs"]).reshape(B, L, H).__setitem__((1, L - 1, 0), 0.0))
    F["frame_past_len_written"] = ("two_v2", (2, 28), lambda b: R.inner(b["scores1"]).reshape(B, L, 9).__setitem__(
        (int(np.argmin(R.fixture(c, (2, 28))[0]["mem"][1]["len"])), 0, 8), 0.0))
    F["input_written"] = ("two_v2", (2, 28), lambda b: R.inner(b["keys0"]).__setitem__(0, 0.0))
    F["token_wrong"] = ("two_v2", (2, 28), lambda b: R.iview(b["fed"]).__setitem__(B * L - 1, 0))
    F["greedy_id_wrong"] = ("two_v2", (1, 41), lambda b: R.iview(b["ids"]).__setitem__(0, 40))
    F["greedy_steplen_wrong"] = ("two_v2", (1, 41), lambda b: R.iview(b["steplen"]).__setitem__(0, 3))
    F["greedy_unfinished_wrong"] = ("two_v2", (1, 41), lambda b: R.iview(b["n_unfinished"]).__setitem__(0, 0))
    return F


BUFFER_FAULTS = _buffer_faults()


@pytest.mark.parametrize("fault", sorted(BUFFER_FAULTS))
def test_checker_rejects_a_damaged_buffer(fault):
    name, key, damage = BUFFER_FAULTS[fault]
    case = R.BY_NAME[name]
    inp, ref, noise, before, good = _bufs(case, key)
    assert R.check(case, key, inp, ref, noise, before, good, again=good, split=good) is None
    bad = {k: a.copy() for k, a in good.items()}
    damage(bad)
    assert R.check(case, key, inp, ref, noise, before, bad) is not None, fault


@pytest.mark.parametrize("which", ["again", "split"])
def test_checker_rejects_one_bit_of_a_repeat_or_a_split_call(which):
    case, key = R.BY_NAME["bahdanau"], (2, 28)
    inp, ref, noise, before, good = _bufs(case, key)
    other = {k: a.copy() for k, a in good.items()}
    R.inner(other["ctx0"]).view(np.uint32)[17] ^= np.uint32(1)
    assert R.check(case, key, inp, ref, noise, before, good, **{which: other}) is not None
    # scratch may differ between calls
    other = {k: a.copy() for k, a in good.items()}
    R.inner(other["state"])[0] = 3.0
    assert R.check(case, key, inp, ref, noise, before, good, **{which: other}) is None


def test_checker_reads_the_error_word_and_accepts_either_pstat_form():
    case, key = R.BY_NAME["two_q32"], (2, 28)
    inp, ref, noise, before, good = _bufs(case, key)
    assert R.check(case, key, inp, ref, noise, before, good, err_word=1) is not None
    # the per-step form records one (max, sum) pair per chunk: the same distribution split over the chunks must pass
    per = {k: a.copy() for k, a in good.items()}
    M = case.mems[1]
    p = R.inner(per["pstat1"]).reshape(case.L, 2, M.nchunk, case.B)
    lse = p[:, 0, 0].copy()
    p[:, 0, 0], p[:, 1, 0] = lse - 1.0, np.float32(np.e) * 0.25
    p[:, 0, 1], p[:, 1, 1] = lse - 2.0, np.float32(np.e ** 2) * 0.75
    assert R.check(case, key, inp, ref, noise, before, per) is None
    p[:, 1, 1] *= 1.01
    assert R.check(case, key, inp, ref, noise, before, per) is not None


# ---- (d) the plan comparison ------------------------------------------------------------------------------------------------------------
def test_plan_matches_on_hand_made_records():
    case, key = R.BY_NAME["two_v2"], (2, 41)
    rec = dict(form="fused", variant=2, rows_per_group=8, v64=1, launches=1, quarter=(33, 3), lds_bytes=12345)
    assert R.plan_matches(rec, R.expected_plan(case, key, 1, False))
    assert R.plan_matches(dict(rec, v64=0), R.expected_plan(case, key, 1, True))
    for field, wrong in (("variant", 1), ("rows_per_group", 16), ("v64", 0), ("launches", 2), ("quarter", (3, 33)), ("form", "per_step")):
        assert not R.plan_matches(dict(rec, **{field: wrong}), R.expected_plan(case, key, 1, False)), field
    ps = dict(form="per_step", variant=-1, rows_per_group=0, v64=0, launches=case.L, quarter=(0, 0), lds_bytes=0)
    for fused, bwd in ((0, False), (0, True), (2, True), (3, False)):
        assert R.expected_plan(case, key, fused, bwd) == "per_step"
        assert R.plan_matches(ps, "per_step") and not R.plan_matches(rec, "per_step")
    assert not R.plan_matches(ps, R.expected_plan(case, key, 1, False))
    full = R.BY_NAME["lds_full"]
    want = R.expected_plan(full, (2, 41), 1, True)
    assert want["lds_bytes"] == 163584 and R.expected_plan(full, (2, 41), 1, False)["lds_bytes"] == 163328
    assert not R.plan_matches(dict(form="fused", variant=1, rows_per_group=8, v64=0, launches=1, quarter=(19, 125), lds_bytes=163328), want)
    assert R.expected_plan(R.BY_NAME["q129"], (2, 28), 1, False) == "per_step"


# ---- (e) the library's plan, which needs no GPU -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,key", ALL_KEYS, ids=["%s-mode%d-V%d" % (n, k[0], k[1]) for n, k in ALL_KEYS])
def test_library_plan_names_the_row(name, key):
    from avsr_tf1_amd import ops
    case = R.BY_NAME[name]
    assert ops.attn_rnn_fused_ws_floats(case.B, len(case.mems)) == R.fused_ws_floats(case.B, len(case.mems))
    for fused in R.FUSED_SETTINGS:
        for bwd in ((False,) if key[0] == 1 else (False, True)):
            rec, want = R.plan(case, key, fused, bwd), R.expected_plan(case, key, fused, bwd)
            assert R.plan_matches(rec, want), (fused, bwd, rec, want)


def test_library_plan_declines_as_the_calls_do():
    """Without a sync scratch or a workspace every plan is per-step; a descriptor the calls refuse is refused with the same code."""
    from avsr_tf1_amd import ops
    from avsr_tf1_amd._lib import AvsrError
    case, key = R.BY_NAME["two_v2"], (2, 28)
    d = R.descriptor(case, key, lambda n: 64)
    ops._L().avsr_rnn_set_persistent(None, 0)
    assert ops.attn_rnn_plan(d)["form"] == "per_step"                       # no sync scratch registered
    nows = R.descriptor(case, key, lambda n: 64, with_ws=False)
    d.labels = None
    try:
        ops._L().avsr_rnn_set_persistent(64, 1 << 20)
        assert ops.attn_rnn_plan(nows)["form"] == "per_step" and ops.attn_rnn_plan(nows, bwd=True)["form"] == "per_step"
        with pytest.raises(AvsrError, match="code -1"):
            ops.attn_rnn_plan(d)                                             # mode 2 without labels: AVSR_ERR_ARG, as avsr_attn_rnn_fwd
        ops._L().avsr_rnn_set_persistent(64, 300)                            # too few sync words for either kernel
        d.labels = 64
        assert ops.attn_rnn_plan(d)["form"] == "per_step" and ops.attn_rnn_plan(d, bwd=True)["form"] == "per_step"
    finally:
        ops._L().avsr_rnn_set_persistent(None, 0)


def _gru_two_layer_descriptor():
    """A GRU block with one layer above the attention-fed cell and no mechanism, by hand: every pointer either call needs is a fake
    non-NULL address (avsr_attn_rnn_plan only tests pointers for NULL)."""
    from avsr_tf1_amd._lib import AttnRnn
    d = AttnRnn()
    d.B, d.L, d.H, d.E, d.n_mech, d.mode, d.cell, d.n_extra = 2, 3, 4, 4, 0, 0, 1, 1
    for f in ("steplen", "wt", "w", "bias", "gates", "cs", "cell_out", "state", "dgates", "dstate", "wt2", "w2", "bias2", "rh_seq", "dgates2", "out0"):
        setattr(d, f, 64)
    X = d.extra[0]
    for f in ("wt", "w", "bias", "gates", "cs", "out", "state", "dgates", "dstate", "wt2", "w2", "bias2", "rh_seq", "dgates2"):
        setattr(X, f, 64)
    X.cell_id = 1
    return d


def test_library_plan_checks_the_gru_layers_of_both_passes():
    """What a GRU layer needs is asked before anything is queued, so the plan answers it too: the candidate kernel and the r*h record of
    the forward pass, the transposed candidate kernel and d(candidate) of the BPTT, for the block's own cell and for a layer above it."""
    from avsr_tf1_amd import ops
    from avsr_tf1_amd._lib import AvsrError
    ops._L().avsr_rnn_set_persistent(None, 0)
    d = _gru_two_layer_descriptor()
    assert ops.attn_rnn_plan(d)["form"] == "per_step" and ops.attn_rnn_plan(d, bwd=True)["form"] == "per_step"
    for where, field, bwd in (("extra", "w2", True), ("extra", "dgates2", True), ("block", "w2", True), ("block", "dgates2", True),
                              ("extra", "wt2", False), ("extra", "rh_seq", False)):
        d = _gru_two_layer_descriptor()
        setattr(d.extra[0] if where == "extra" else d, field, None)
        with pytest.raises(AvsrError, match="code -1"):                     # AVSR_ERR_ARG
            ops.attn_rnn_plan(d, bwd=bwd)
