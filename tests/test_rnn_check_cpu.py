"""The encoder RNN conformance suite judged without a GPU (tests/ref_rnn.py holds the reference, the case table and the checker):
  (a) the reference agrees with oracle.dynamic_rnn + autograd to 1e-10, every cell kind, forward and reverse, with and without dropout;
  (b) every case of the table meets the conditions that make it a test (cells clip, gates saturate, nothing sits on the clip's kink, the
      fp32 twin's noise stays under the cap, the len vector holds what the row promises);
  (c) avsr_rnn_plan -- the library's own dispatch on its dry path -- sends every case to the form its row names, every form of the enum
      is named by a case in each direction it exists in, and the benchmark encoders plan to the forms DESIGN.md claims;
  (d) the checker rejects every listed mutation of a correct result (and accepts the correct one, and the fp32 twin)."""

import numpy as np
import pytest
import torch

import ref_rnn as R

BY_NAME = {c.name: c for c in R.CASES}
IDS = [c.name for c in R.CASES]


# ---- (a) the reference against the oracle ---------------------------------------------------------------------------------------------
def _to_tf(We, G):
    """engine layout (columns G*unit + gate) -> TF layout (columns gate*H + unit), differentiable"""
    K, GH = We.shape
    return We.view(K, GH // G, G).transpose(1, 2).reshape(K, GH)


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("kind", ["lstm", "gru", "lstm_residual", "gru_residual"])
def test_reference_agrees_with_the_oracle(kind, reverse, drop):
    from oracle import avsr_oracle as O
    cell = kind.split("_")[0]
    res = kind.endswith("residual")
    units = (8, 8, 12) if res else (8, 12)
    B, T, F = 5, 6, R.F_IN
    dr = R.Drop(consumer_keep=1.0, seed=41) if drop else None
    st = R.Stack(units, T, reverse=reverse, cell=cell, residual=(1,) if res else (), drop=dr, cell_id_base=5)
    rng = np.random.default_rng(3 + reverse)
    lens = np.array([T, 1, 0, 4, 2], np.int64)
    G = 4 if cell == "lstm" else 2
    leaves = dict(x=torch.tensor(rng.standard_normal((B, T, F)), requires_grad=True))
    d = dict(W=[], b=[], W2=[], b2=[], lens=lens)
    for l, (H, i) in enumerate(zip(units, R.in_dims(st))):
        for name, shape in (("W", (i + H, G * H)), ("b", (G * H,))) + ((("W2", (i + H, H)), ("b2", (H,))) if cell == "gru" else ()):
            leaves["%s%d" % (name, l)] = torch.tensor(rng.standard_normal(shape) * (0.1 if name[0] == "b" else 1.5 / np.sqrt(i + H)), requires_grad=True)
            d[name].append(leaves["%s%d" % (name, l)])
    x = leaves["x"]
    xm = x
    if drop:        # layer 0's input mask is the caller's (it precedes the hoisted GEMM): stream cell_id*4 + 0, width F
        idx = np.arange(B * T * F, dtype=np.uint32).reshape(B, T, F)
        xm = x * torch.tensor((O.uniform01(dr.seed, st.cell_id_base * 4, idx) < np.float32(dr.keep_in)) / dr.keep_in)
    d["z0"] = (xm @ d["W"][0][:F]).reshape(B, T, units[0], G)
    if cell == "gru":
        d["zc0"] = xm @ d["W2"][0][:F]
    Ht = units[-1]
    d["R_out"], d["R_xt"] = rng.standard_normal((B, T, Ht)), rng.standard_normal((B, T, Ht))
    d["R_h"], d["R_c"] = rng.standard_normal((B, Ht)), rng.standard_normal((B, Ht))
    mine = R.run_stack(st, B, d)                                  # runs loss.backward()
    g_mine = {k: v.grad.clone() for k, v in leaves.items()}
    for v in leaves.values():
        v.grad = None

    P = {}
    for l in range(len(units)):
        if cell == "lstm":
            P["s/l%d/kernel" % l], P["s/l%d/bias" % l] = _to_tf(d["W"][l], 4), _to_tf(d["b"][l][None], 4)[0]
        else:
            P["s/l%d/gates_kernel" % l], P["s/l%d/gates_bias" % l] = _to_tf(d["W"][l], 2), _to_tf(d["b"][l][None], 2)[0]
            P["s/l%d/cand_kernel" % l], P["s/l%d/cand_bias" % l] = d["W2"][l], d["b2"][l]
    cells = [O._Cell(P, "s/l%d" % l, cell, u) for l, u in enumerate(units)]
    lt = torch.tensor(lens)
    if drop:
        for l, c in enumerate(cells):
            c.set_dropout((dr.keep_in, dr.keep_state, dr.keep_out), st.cell_id_base + l, T, dr.seed, lt, bool(reverse))
    xin = O._reverse_sequence(x, lt) if reverse else x
    step = O._stack_step(cells, "residual", P, "s") if res else O._stack_step(cells)
    if res:       # the oracle wraps every layer above the first; this suite's stack wraps layer 1 only
        def step(xx, states, t=0, _cells=cells):
            new = []
            for l, (c, s) in enumerate(zip(_cells, states)):
                y, ns = c(xx, s, t)
                xx = y + xx if l == 1 else y
                new.append(ns)
            return xx, tuple(new)
    outs, fin = O.dynamic_rnn(step, tuple(c.zero_state(B, torch.float64) for c in cells), xin, lt)
    if reverse:
        outs = O._reverse_sequence(outs, lt)
    loss = (outs * torch.tensor(d["R_out"])).sum() + (fin[-1][-1] * torch.tensor(d["R_h"])).sum()
    if drop:
        loss = loss + (outs * torch.tensor(d["R_xt"])).sum()      # consumer_keep 1: xt_seq of the top layer is its output
    if cell == "lstm":
        loss = loss + (fin[-1][0] * torch.tensor(d["R_c"])).sum()
    loss.backward()
    top = mine["layers"][-1]
    assert np.abs(top["out"] - outs.detach().numpy()).max() < 1e-10
    assert np.abs(top["h_final"] - fin[-1][-1].detach().numpy()).max() < 1e-10
    if cell == "lstm":
        assert np.abs(top["c_final"] - fin[-1][0].detach().numpy()).max() < 1e-10
    assert abs(float(mine["loss"].detach()) - float(loss.detach())) < 1e-10 * max(1.0, abs(float(loss.detach())))
    for k, v in leaves.items():
        assert v.grad is not None and float(v.grad.abs().max()) > 0, k
        assert float((g_mine[k] - v.grad).abs().max()) < 1e-10, k


# ---- (b) conditions on every case -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IDS)
def test_case_meets_its_conditions(name):
    case = BY_NAME[name]
    inp, ref, noise = R.fixture(case)
    c = R.conditions(case, ref, noise)
    print(name, c)
    lstm = all(s.cell == "lstm" for s in case.stacks)
    assert c["near"] > 1e-4, c                          # the clip's gradient is discontinuous at +-1: fp32 and fp64 must take the same side
    if lstm and case.clips:
        assert c["clipped"] >= 0.01, c
    assert c["saturated"] >= 0.05, c
    assert c["saturated_sigmoid"] >= 0.02, c            # ... and not only through tanh values below 0.05
    assert c["noise_rel"] <= R.NOISE_CAP, c
    for si, st in enumerate(case.stacks):
        lens = R.lens_of(case, si)
        assert st.T >= 1 and st.T <= 9
        assert case.B % (16 if case.B > 64 else 8) != 0             # B never fills its last group
        if st.lens == "null":
            assert lens is None and (ref[si]["lens"] == st.T).all()
        else:
            assert {0, 1, st.T} <= set(lens.tolist()) and lens.max() <= st.T
    if len(case.stacks) == 2 and case.name.startswith("two_T"):
        assert case.stacks[0].T != case.stacks[1].T and not np.array_equal(R.lens_of(case, 0), R.lens_of(case, 1))


def test_table_holds_odd_and_even_T():
    Ts = {s.T for c in R.CASES for s in c.stacks}
    assert any(t & 1 for t in Ts) and any(not (t & 1) for t in Ts if t > 1)


# ---- (c) the plan ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IDS)
def test_plan_names_the_form_of_every_case(name):
    case = BY_NAME[name]
    for bwd, table in ((False, case.fwd), (True, case.bwd)):
        for mode in (0, 1, 3, 6):
            recs = R.plan(case, bwd, mode)
            assert R.plan_matches(recs, table[mode]), (name, "bwd" if bwd else "fwd", mode, table[mode], recs)
            for r in recs:
                assert (r["form"] == "per_step") == (r["rows_per_slice"] == 0) and r["launches"] >= 1
    if case.small_scratch:
        assert R.plan(case, True, 3)[0]["form"] == "bwd_ksplit"
        assert R.plan(case, True, 3, R.SMALL_SCRATCH)[0]["form"] == "bwd_unit"


def _forms(table):
    out = set()
    for c in R.CASES:
        for mode in c.modes:
            w = getattr(c, table)[mode]
            for e in (w if isinstance(w, list) else [w]):
                out.add(e if isinstance(e, str) else e[0])
    return out


def test_every_form_is_named_by_a_case():
    from avsr_tf1_amd import ops
    assert _forms("fwd") == {f for f in ops.RNN_FORMS if f.startswith("fwd_")} | {"per_step"}
    assert _forms("bwd") == {f for f in ops.RNN_FORMS if f.startswith("bwd_")} | {"per_step"}
    # ... with and without crossing edges, one and two top tiles, one launch per stack, more than one slice
    recs = [r for c in R.CASES for m in c.modes if m for r in R.plan(c, True, m)]
    for form in ("bwd_ksplit", "bwd_unit"):
        assert {r["crossing_edges"] > 0 for r in recs if r["form"] == form} == {False, True}
    assert {r["top_tiles"] for r in recs if r["form"] == "bwd_unit"} == {1, 2}
    assert {r["launches"] > 1 for r in recs if r["form"] != "per_step"} == {False, True}
    assert any(len(R.plan(c, False, 3)) == 2 for c in R.CASES) and any(len(R.plan(c, True, 3)) == 2 for c in R.CASES)
    # a BPTT that goes per-step after a persistent forward
    assert any(R.plan(c, False, 3)[0]["form"] != "per_step" and R.plan(c, True, 3)[0]["form"] == "per_step" for c in R.CASES)


def test_benchmark_encoders_plan_to_the_forms_design_md_claims():
    """bench.py's workloads (dropout on, so hs_seq / xt_seq are given): c4 = video 1 x 256 (T 75) + audio 3 x 256 (T 500), B = 64;
    c2 = the two directions of 3 x 256 audio; c5 = the plain layers under the attentive top, video 1 x 256 + audio 2 x 256, B = 128."""
    dr = R.Drop()
    c4 = R.Case("c4", 64, (R.Stack((256,), 75, drop=dr), R.Stack((256, 256, 256), 500, drop=dr, cell_id_base=11)), {}, {})
    assert R.plan_matches(R.plan(c4, False, 3), ("fwd_xcd8_q4", dict(stacks=2, wg_per_xcd=96, launches=1, rows_per_group=8)))
    assert R.plan_matches(R.plan(c4, True, 3), ("bwd_ksplit", dict(stacks=2, launches=1, crossing_edges=(1, 9), wg_per_xcd=(33, 64))))
    c2 = R.Case("c2", 64, (R.Stack((256, 256, 256), 500, drop=dr), R.Stack((256, 256, 256), 500, reverse=1, drop=dr, cell_id_base=11)), {}, {})
    assert R.plan_matches(R.plan(c2, False, 3), ("fwd_parts", dict(stacks=2, wg_per_xcd=80, rows_per_group=16, launches=1)))
    assert R.plan_matches(R.plan(c2, True, 3), [("bwd_ksplit", dict(stacks=1, launches=1, crossing_edges=(1, 9)))] * 2)
    c5 = R.Case("c5", 128, (R.Stack((256,), 75, drop=dr), R.Stack((256, 256), 500, drop=dr, cell_id_base=11)), {}, {})
    assert R.plan_matches(R.plan(c5, False, 3), ("fwd_xcd16", dict(stacks=2, wg_per_xcd=64, launches=1, rows_per_slice=128)))
    assert R.plan_matches(R.plan(c5, True, 3), ("bwd_ksplit_solo", dict(stacks=2, wg_per_xcd=64, launches=1, crossing_edges=0)))


def test_plan_leaves_the_installed_state_alone_and_rejects_bad_arguments():
    from avsr_tf1_amd import _lib, ops
    case = BY_NAME["u32_48_32_b19/fw"]
    a = R.plan(case, True, 3)
    assert R.plan(case, True, 0)[0]["form"] == "per_step" and R.plan(case, True, 3) == a
    st = R.descriptors(case, lambda k: 64)
    st[0].B = 0
    with pytest.raises(_lib.AvsrError):
        ops.rnn_plan(st)
    # nine layers in all: more than one per-step launch holds.  avsr_rnn_bwd refuses that before it tries anything (and so does the plan);
    # avsr_rnn_fwd runs them as one persistent launch per stack, or refuses when it would need the per-step form
    nine = R.Case("nine", 9, tuple(R.Stack((32, 48, 32), 5, cell_id_base=8 * i) for i in range(3)), {}, {})
    assert [r["form"] for r in R.plan(nine, False, 3)] == ["fwd_xcd8"] * 3
    for bwd, mode in ((True, 3), (True, 0), (False, 0)):
        with pytest.raises(_lib.AvsrError):
            R.plan(nine, bwd, mode)
    # the per-step form counts the wavefront's launches: T + layers - 1, two phases for a GRU
    assert R.plan(case, False, 0)[0]["launches"] == 8 + 3 - 1
    assert R.plan(BY_NAME["gru/fw"], False, 3)[0]["launches"] == 2 * (6 + 2 - 1)
    assert R.plan(BY_NAME["two_T/fw"], True, 0)[0]["launches"] == 9 + 2 - 1


# ---- (d) the checker ------------------------------------------------------------------------------------------------------------------
def _judge(case, after, ref=None):
    inp, r64, noise = R.fixture(case)
    return R.check(case, inp, r64, noise, R.initial_buffers(case, inp, r64), after)


@pytest.mark.parametrize("name", IDS)
def test_checker_accepts_the_reference_and_its_fp32_twin(name):
    case = BY_NAME[name]
    inp, r64, noise = R.fixture(case)
    assert _judge(case, R.expected_buffers(case, inp, r64)) is None
    assert _judge(case, R.expected_buffers(case, inp, R.reference(case, inp, torch.float32))) is None


B19, B19R, U8, DROP, BIDI, NUL = "u32_48_32_b19/fw", "u32_48_32_b19/rv", "u8_24_40/fw", "drop_b19/fw", "bidi_b17", "len_null/fw"
# name -> (case, fault of the reference, quantities the first offence may name)
REF_FAULTS = {
    "state not carried through past len": (B19, {"no_carry": 1}, ("h_final", "c_final")),
    "reverse walked from T-1": (B19R, {"rev_from_T": 1}, None),
    "a row computed with its neighbour's length": (B19, {"nbr_len": None}, None),
    "forget bias left out": (B19, {"no_forget_bias": 1}, ("gates",)),
    "clip left out": (B19, {"no_clip": 1}, ("gates", "cs")),       # (the gates of the next step are judged before this step's cs)
    "last k-term of the recurrent product dropped (in_dim % 16 != 0)": (U8, {"drop_k": 1}, ("gates", "dgates")),     # (layer 0's dgates are judged before layer 1's gates)
    "x operand of step t+1 used at odd t": (B19, {"x_next_odd": 1}, ("gates", "dgates")),
    "dh_final injected at T-1": (B19, {"dh_at_T": 1}, ("dgates",)),
    "a state-dropout mask taken from the output stream": (DROP, {"state_mask_from_out": 1}, None),
    "operands rounded to bf16": (B19, {"bf16": 1}, ("gates",)),
}


@pytest.mark.parametrize("fault", list(REF_FAULTS))
def test_checker_rejects_a_faulty_computation(fault):
    name, mut, quantities = REF_FAULTS[fault]
    case = BY_NAME[name]
    inp, r64, _ = R.fixture(case)
    if "nbr_len" in mut:
        lens = r64[0]["lens"]
        mut = {"nbr_len": int(np.flatnonzero((lens[:-1] != lens[1:]) & (lens[:-1] > 1) & (lens[1:] > 1))[0])}
    if "drop_k" in mut:
        assert R.in_dims(case.stacks[0])[mut["drop_k"]] % 16 != 0
    bad = R.reference(case, inp, mut=(0, mut))
    off = _judge(case, R.expected_buffers(case, inp, bad))
    print(fault, off)
    assert off is not None
    if quantities:
        assert off[2] in quantities, off


def _bufs(name):
    case = BY_NAME[name]
    inp, r64, _ = R.fixture(case)
    return case, r64, R.expected_buffers(case, inp, r64)


def _seq(case, bufs, si, l):
    key, ld, col = R.out_place(case, si, l)
    return R.inner(bufs[key]).reshape(case.B, case.stacks[si].T + 2, ld), col


def _short_row(ref, si=0, least=1):
    lens = ref[si]["lens"]
    return int(np.flatnonzero((lens >= least) & (lens < lens.max()))[0])


def test_checker_rejects_a_nonzero_output_row_past_len():
    case, ref, bufs = _bufs(B19)
    b = _short_row(ref)
    o, col = _seq(case, bufs, 0, 1)
    o[b, 1 + ref[0]["lens"][b], col + 3] = 1e-30
    off = _judge(case, bufs)
    assert off and off[:3] == (0, 1, "out") and off[3] == b and off[4] == ref[0]["lens"][b] and off[5] == 3, off


def test_checker_rejects_swapped_rows_of_a_group():
    case, ref, bufs = _bufs(B19)
    g = R.inner(bufs[(0, 2, "gates")]).reshape(case.B, -1)
    g[[1, 9]] = g[[9, 1]]
    assert _judge(case, bufs)[:3] == (0, 2, "gates")
    case, ref, bufs = _bufs(B19)
    o, col = _seq(case, bufs, 0, 2)
    o[[2, 10]] = o[[10, 2]]
    assert _judge(case, bufs)[:3] == (0, 2, "out")


def test_checker_rejects_two_swapped_gates_of_one_unit():
    case, ref, bufs = _bufs(B19)
    b = _short_row(ref, least=2)
    g = R.inner(bufs[(0, 0, "gates")]).reshape(case.B, 8, 32, 4)
    g[b, 1, 5, [0, 3]] = g[b, 1, 5, [3, 0]]
    assert _judge(case, bufs)[:6] == (0, 0, "gates", b, 1, 5)
    case, ref, bufs = _bufs(B19)
    g = R.inner(bufs[(0, 1, "dgates")]).reshape(case.B, 8, 48, 4)
    g[b, 0, 7, [1, 2]] = g[b, 0, 7, [2, 1]]
    assert _judge(case, bufs)[:6] == (0, 1, "dgates", b, 0, 7)


def test_checker_rejects_a_nonzero_dgates_past_len():
    case, ref, bufs = _bufs(B19)
    b = _short_row(ref)
    g = R.inner(bufs[(0, 2, "dgates")]).reshape(case.B, 8, 32, 4)
    g[b, 7, 31, 2] = 1e-30
    off = _judge(case, bufs)
    assert off[:6] == (0, 2, "dgates", b, 7, 31) and "zero" in off[6], off


def test_checker_rejects_one_float_out_of_place():
    # a guard slot
    for slot in (0, 9):
        case, ref, bufs = _bufs(B19)
        o, col = _seq(case, bufs, 0, 0)
        o[4, slot, 1] = 1.0
        off = _judge(case, bufs)
        assert off[:3] == (0, 0, "out") and "guard slot" in off[6], off
    case, ref, bufs = _bufs(DROP)
    R.inner(bufs[(0, 1, "hs")]).reshape(case.B, 10, 48)[3, 9, 47] = 1.0
    assert "guard slot" in _judge(case, bufs)[6]
    # the neighbouring column block of a shared buffer: the other stack's output, or a column that belongs to nobody
    case, ref, bufs = _bufs(BIDI)
    o, col = _seq(case, bufs, 0, 2)
    b = int(np.argmax(ref[1]["lens"]))
    o[b, 1, 16] = 1.0
    assert _judge(case, bufs)[:3] == (1, 2, "out")
    case, ref, bufs = _bufs(NUL)
    o, col = _seq(case, bufs, 0, 2)
    assert col == 4 and o.shape[2] == 40
    o[7, 3, 36] = 1.0
    off = _judge(case, bufs)
    assert off[:3] == (0, 2, "out") and "outside every block" in off[6], off
    # the NaN band, on either side of a record and of a scratch
    for key, word in (((0, 1, "cs"), R.GUARD - 1), ((0, 1, "cs"), -R.GUARD), ((0, 0, "state"), -1), ((0, 2, "dstate"), 0)):
        case, ref, bufs = _bufs(B19)
        bufs[key][word] = 1.0
        off = _judge(case, bufs)
        assert off[:3] == key and "guard band" in off[6], off


def test_checker_rejects_a_raised_error_word_a_written_input_and_a_second_call_that_differs():
    case, ref, bufs = _bufs(B19)
    inp, r64, noise = R.fixture(case)
    before = R.initial_buffers(case, inp, r64)
    assert R.check(case, inp, r64, noise, before, bufs, err_word=1)[2] == "sync"
    again = {k: v.copy() for k, v in bufs.items()}
    assert R.check(case, inp, r64, noise, before, bufs, again=again) is None
    again[(0, 1, "dgates")][R.GUARD + 17] = np.nextafter(again[(0, 1, "dgates")][R.GUARD + 17], np.float32(1))
    assert "second identical call" in R.check(case, inp, r64, noise, before, bufs, again=again)[6]
    R.inner(bufs[(0, 2, "dout")])[5] += 1.0
    assert R.check(case, inp, r64, noise, before, bufs)[2] == "dout"


def test_tolerance_rule():
    noise = {"gates": (1e-7, 1.0), "dgates": (1e-4, 30.0)}
    assert R.tolerance("gates", noise) == R.T_SUITE
    assert R.tolerance("gates", {"gates": (1e-5, 1.0)}) == 8e-5
    assert R.tolerance("dgates", {"dgates": (1e-7, 30.0)}, 30.0) == pytest.approx(6e-3)
    assert R.tolerance("dgates", noise, 0.5) == pytest.approx(8e-4)
