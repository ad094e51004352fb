"""Conformance of avsr_rnn_fwd / avsr_rnn_bwd over every dispatch form ("The contract of avsr_rnn_fwd / avsr_rnn_bwd").

One test per (case of tests/ref_rnn.py's table, mode of avsr_rnn_set_persistent_mode): forward then BPTT through ops.rnn_fwd / ops.rnn_bwd
on RnnStack descriptors whose every buffer sits inside a NaN band.  Before anything is compared the form is asserted: avsr_rnn_plan must
name what the case's row names, and the event profiler must show exactly the planned number of rnn_persist_fwd / rnn_persist_bwd launches
and no step_lstm_fwd / step_lstm_bwd launch (for a planned per-step form the other way round).  Then tests/ref_rnn.py's checker judges
the buffers against the fp64 reference: records, outputs, final states and dgates within max(T_suite, 8 x noise), exact zeros past len
and in the guard slots, foreign columns and the NaN bands bit-unchanged, the sticky error word 0, a second identical call bit-equal.
tests/test_rnn_check_cpu.py shows on the CPU that this checker rejects the faults a kernel of this kind can have."""
import numpy as np
import pytest
import torch

import ref_rnn as R

pytestmark = pytest.mark.gpu

PARAMS = [(c.name, m, False) for c in R.CASES for m in c.modes] + [(c.name, 3, True) for c in R.CASES if c.small_scratch]


def _upload(case, inp, before):
    dev = {k: torch.from_numpy(v).cuda() for k, v in before.items()}
    for si, st in enumerate(case.stacks):
        d = inp[si]
        if d["lens"] is not None:
            dev[("len", si)] = torch.tensor(d["lens"], dtype=torch.int32).cuda()
        dev[("dh_final", si)] = torch.tensor(d["R_h"], dtype=torch.float32).cuda()
        dev[("dc_final", si)] = torch.tensor(d["R_c"], dtype=torch.float32).cuda()
        if st.drop:
            dev[("seed", si)] = torch.tensor([st.drop.seed], dtype=torch.int32).cuda()
        for l in range(len(st.units)):
            for w, wt, b, src, bsrc in (("w", "wt", "bias", "W", "b"), ("w2", "wt2", "bias2", "W2", "b2")):
                if d[src]:
                    dev[(w, si, l)] = torch.from_numpy(d[src][l]).cuda()
                    dev[(wt, si, l)] = dev[(w, si, l)].t().contiguous()
                    dev[(b, si, l)] = torch.from_numpy(d[bsrc][l]).cuda()
    return dev


def _addr(dev, before):
    return lambda key: dev[key].data_ptr() + (4 * R.GUARD if key in before else 0)


def _run(case, inp, before, mode, small):
    """Forward + BPTT from the initial buffers: (forward counts, BPTT counts, error word, buffers afterwards)."""
    from avsr_tf1_amd import ops
    from avsr_tf1_amd.ops import _L
    dev = _upload(case, inp, before)
    stacks = R.descriptors(case, _addr(dev, before))
    tiny = torch.zeros(R.SMALL_SCRATCH, device="cuda") if small else None
    try:
        ops.rnn_set_persistent(bool(mode), mode=max(mode, 1))
        if small:
            _L().avsr_rnn_set_persistent_scratch(tiny.data_ptr(), tiny.numel())
        counts = []
        for fn in (ops.rnn_fwd, ops.rnn_bwd):
            ops.prof_begin()
            fn(stacks)
            counts.append(ops.prof_end())
        torch.cuda.synchronize()
        err = int(ops.rnn_persistent_error())
    finally:
        if small:
            _L().avsr_rnn_set_persistent_scratch(None, 0)
        ops.rnn_set_persistent(False)
    return counts[0], counts[1], err, {k: dev[k].cpu().numpy() for k in before}


@pytest.mark.parametrize("name,mode,small", PARAMS, ids=["%s-mode%d%s" % (n, m, "-small_scratch" if s else "") for n, m, s in PARAMS])
def test_rnn_conformance(name, mode, small):
    from avsr_tf1_amd import ops
    case = {c.name: c for c in R.CASES}[name]
    inp, ref, noise = R.fixture(case)
    before = R.initial_buffers(case, inp, ref)
    scratch = R.SMALL_SCRATCH if small else 64 << 20
    plans = [R.plan(case, bwd, mode, scratch) for bwd in (False, True)]
    assert R.plan_matches(plans[0], case.fwd[mode]), plans[0]
    assert R.plan_matches(plans[1], [("bwd_unit", {})] * len(plans[1]) if small else case.bwd[mode]), plans[1]

    fwd, bwd, err, after = _run(case, inp, before, mode, small)
    # the form: the planned launches, and none of the other kind
    for recs, cnt, pk, sk in ((plans[0], fwd, "rnn_persist_fwd", "step_lstm_fwd"), (plans[1], bwd, "rnn_persist_bwd", "step_lstm_bwd")):
        planned = sum(r["launches"] for r in recs)
        if recs[0]["form"] == "per_step":
            assert (cnt[pk][0], cnt[sk][0]) == (0, planned), (recs, cnt[pk], cnt[sk])
        else:
            assert (cnt[pk][0], cnt[sk][0]) == (planned, 0), (recs, cnt[pk], cnt[sk])
    _, _, err2, again = _run(case, inp, before, mode, small)
    log = []
    off = R.check(case, inp, ref, noise, before, after, again=again, err_word=err or err2, log=log)
    worst = {}
    for _si, _l, q, e, tol in log:
        worst[q] = max(worst.get(q, (0.0, 0.0)), (e, tol))
    print("%s mode %d%s: fwd %s, bwd %s" % (name, mode, " small scratch" if small else "", plans[0][0]["form"], plans[1][0]["form"]))
    for q, (e, tol) in sorted(worst.items()):
        print("  %-8s engine error %.3e  noise %.3e  bound %.3e" % (q, e, noise[q][0], tol))
    assert off is None, off
