"""Conformance of avsr_attn_rnn_fwd / avsr_attn_rnn_bwd over every fused dispatch form ("The contract of avsr_attn_rnn_fwd /
avsr_attn_rnn_bwd").

One test per (row of tests/ref_dec.py's table, mode, vocabulary, avsr_attn_rnn_set_fused setting): forward then BPTT on an AttnRnn
descriptor whose every buffer sits inside a NaN band.  Before anything is compared the form is asserted: avsr_attn_rnn_plan must name what
the row names (variant, rows per group, quarter widths, slices, the 64-symbol template, where the row pins it the LDS bytes), and the event
profiler must show exactly the planned number of fused launches of the right class (decoder, or attentive by prof_tag) and no per-step
cell or attention launch of the block -- for a planned per-step form the other way round.  Then tests/ref_dec.py's checker judges the
buffers against the fp64 reference within max(T_suite, 8 x noise): records, outputs, logits, states and the BPTT outputs, tokens exactly,
zeros at dead steps, rows and frames a call must not write, inputs and the NaN bands bit-unchanged, the sticky error word 0, a second
identical call bit-equal, and (rows marked split) a forward issued as [0, 2) then [2, L) bit-equal to one call.
tests/test_dec_check_cpu.py shows on the CPU that this checker rejects the faults a kernel of this kind can have."""
import pytest
import torch

import ref_dec as R

pytestmark = pytest.mark.gpu

PARAMS = [(c.name, m, V, f) for c in R.CASES for (m, V) in c.keys() for f in R.FUSED_SETTINGS]


def _run(case, key, before, fused, split=False):
    """Forward (+ BPTT) from the initial buffers: (plans, forward counts, BPTT counts, error word, buffers afterwards)."""
    from avsr_tf1_amd import ops
    mode = key[0]
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in before.items()}
    desc = R.descriptor(case, key, lambda n: dev[n].data_ptr() + 4 * R.GUARD)
    try:
        ops.rnn_set_persistent(True)
        ops.attn_rnn_set_fused(fused)
        plans = [ops.attn_rnn_plan(desc, bwd=b) for b in ((False,) if mode == 1 else (False, True))]
        counts = []
        ops.prof_begin()
        if split:
            ops.attn_rnn_fwd(desc, 0, 2)
            ops.attn_rnn_fwd(desc, 2, case.L)
        else:
            ops.attn_rnn_fwd(desc, 0, case.L)
        counts.append(ops.prof_end())
        if mode != 1:
            ops.prof_begin()
            ops.attn_rnn_bwd(desc)
            counts.append(ops.prof_end())
        torch.cuda.synchronize()
        err = int(ops.rnn_persistent_error())
    finally:
        ops.attn_rnn_set_fused(1)
        ops.rnn_set_persistent(False)
    return plans, counts, err, {k: dev[k].cpu().numpy() for k in before}


@pytest.mark.parametrize("name,mode,V,fused", PARAMS, ids=["%s-mode%d-V%d-fused%d" % p for p in PARAMS])
def test_dec_conformance(name, mode, V, fused):
    from avsr_tf1_amd import ops
    case, key = R.BY_NAME[name], (mode, V)
    assert ops.attn_rnn_fused_ws_floats(case.B, len(case.mems)) == R.fused_ws_floats(case.B, len(case.mems))
    inp, ref, noise = R.fixture(case, key)
    before = R.initial_buffers(case, key, inp)
    plans, counts, err, after = _run(case, key, before, fused)
    # the form, before any number: the plan is the row's, the launches are the plan's and none of the other kind ran
    tag = "align_persist" if case.prof_tag == 1 else "dec_persist"
    other = "dec_persist" if case.prof_tag == 1 else "align_persist"
    for bwd, (rec, cnt) in enumerate(zip(plans, counts)):
        assert R.plan_matches(rec, R.expected_plan(case, key, fused, bool(bwd))), (bwd, rec, R.expected_plan(case, key, fused, bool(bwd)))
        sfx = "_bwd" if bwd else "_fwd"
        seen = (cnt[tag + sfx][0], cnt[other + sfx][0], cnt["step_lstm" + sfx][0], cnt["attn" + sfx][0])
        if rec["form"] == "fused":
            assert seen == (rec["launches"], 0, 0, 0), (bwd, rec, seen)
        else:
            assert seen == (0, 0, case.L, case.L), (bwd, rec, seen)
    _, _, err2, again = _run(case, key, before, fused)
    split, err3 = None, 0
    if case.split and mode >= 1:
        _, _, err3, split = _run(case, key, before, fused, split=True)
    log = []
    off = R.check(case, key, inp, ref, noise, before, after, again=again, split=split, err_word=err or err2 or err3, log=log)
    worst = {}
    for q, e, tol in log:
        worst[q] = max(worst.get(q, (0.0, 0.0)), (e, tol))
    print("%s mode %d V %d fused %d: fwd %s, bwd %s" % (name, mode, V, fused, plans[0], plans[1] if len(plans) > 1 else None))
    for q, (e, tol) in sorted(worst.items()):
        print("  DECQ %s %d %d %d %-8s engine error %.3e  noise %.3e  bound %.3e" % (name, mode, V, fused, q, e, noise[q][0], tol))
    assert off is None, off
