"""Attention rescoring, the parts that need no GPU: the fp64 reference of tests/ref_rescore.py against torch's cross-entropy, the selection's
tie order and its weight-0 branch, what AVSR's constructor accepts and refuses, and the host-side argument checks of the two C entry
points."""
import os

import numpy as np
import pytest
import torch

import ref_rescore as R
from test_ctc_prefix_cpu import _unit_file
from test_logmel_cpu import _construct


def test_tolerance_is_measured_not_chosen():
    assert 0.0 < R.F32_DEVIATION < 1e-3 and R.TOL_SCORE == 8 * R.F32_DEVIATION
    keys = [k for k, _c in R.kernel_cases()]
    assert len(keys) == len(set(keys)) == 45 + 5 and all(R.kernel_reference(*k).shape == (k[2],) for k in keys)


@pytest.mark.parametrize("V,L,B", [(2, 1, 1), (15, 7, 3), (41, 40, 3), (257, 7, 64)])
def test_seq_logprob_is_minus_the_summed_cross_entropy(V, L, B):
    z, labels, lens = R.kernel_case(V, L, B)
    got = R.seq_logprob(z, labels, lens)
    zt, lt = torch.tensor(z, dtype=torch.float64), torch.tensor(labels, dtype=torch.int64)
    for b in range(B):
        n = int(np.clip(lens[b], 0, L))
        want = -float(torch.nn.functional.cross_entropy(zt[b, :n], lt[b, :n], reduction="sum")) if n else 0.0
        assert np.isclose(got[b], want, rtol=1e-12, atol=1e-12), (b, got[b], want)
    assert np.array_equal(got, R.kernel_reference(V, L, B))
    if B >= 3:
        assert lens[1] == 0 and got[1] == 0.0 and lens[2] > L                # no labels: exactly 0; a length above L is clamped


def test_seq_logprob_peaked_rows_and_labels_out_of_range():
    z, labels, lens = R.kernel_case(31, 7, 3, peaked=True)
    got = R.seq_logprob(z, labels, lens)
    for b in range(3):
        n = int(np.clip(lens[b], 0, 7))
        off = sum(1 for t in range(n) if z[b, t, labels[b, t]] < 0)
        assert abs(got[b] - (-2 * R.PEAK * off)) < 1e-9                     # on the peak: log 1; off it: -160; exp(-160) is below fp64's ulp of 1
    assert np.array_equal(R.seq_logprob_f32(z, labels, lens).astype(np.float64), got)      # ... and float32 gets the same
    bad = np.array(labels)
    bad[0, 0], bad[2, 1] = -1, 31
    out = R.seq_logprob(z, bad, lens)
    assert out[0] == -np.inf and out[2] == -np.inf and out[1] == got[1] and not np.isnan(out).any()


def test_select_orders_by_final_then_by_ctc_rank():
    s_att = np.array([[-3.0, -1.0, -3.0, -1.0, -2.0], [-1.0, -1.0, -1.0, 9.0, 9.0]], np.float32)
    s_ctc = np.array([[-1.0, -2.0, -3.0, -4.0, -np.inf], [-2.0, -4.0, -8.0, -np.inf, -np.inf]], np.float32)
    order, final = R.select(s_att, s_ctc, [4, 3], 0.0)                      # weight 0: s_att alone, the -inf beyond n never met
    assert order.tolist() == [[1, 3, 0, 2, -1], [0, 1, 2, -1, -1]]
    assert final.tolist() == [[-1.0, -1.0, -3.0, -3.0, -np.inf], [-1.0, -1.0, -1.0, -np.inf, -np.inf]]
    order, final = R.select(s_att, s_ctc, [4, 3], 0.5)
    # utterance 0: finals -3.5, -2, -4.5, -3 -> 1, 3, 0, 2; utterance 1: -2, -3, -5
    assert order.tolist() == [[1, 3, 0, 2, -1], [0, 1, 2, -1, -1]]
    assert final.tolist() == [[-2.0, -3.0, -3.5, -4.5, -np.inf], [-2.0, -3.0, -5.0, -np.inf, -np.inf]]
    order, final = R.select(np.array([[-2.0, -1.0, -1.5]], np.float32), np.array([[0.0, -2.0, -1.0]], np.float32), [3], 0.5)
    assert order.tolist() == [[0, 1, 2]] and final.tolist() == [[-2.0, -2.0, -2.0]]            # a three-way tie planted by the weight
    assert not np.isnan(R.select(s_att, s_ctc, [5, 5], 0.0)[1]).any()       # weight 0 forms no product: no 0 * -inf
    order, final = R.select(s_att, s_ctc, [0, 9], 0.0)                      # n is clamped to 0 .. K
    assert order[0].tolist() == [-1] * 5 and (final[0] == -np.inf).all() and sorted(order[1].tolist()) == [0, 1, 2, 3, 4]


def test_avsr_constructs_with_attention_rescoring(tmp_path, monkeypatch):
    from test_gpu_avsr import _dataset
    unit_file, p = _dataset(str(tmp_path), n=3)
    kw = dict(unit="character", unit_file=unit_file, audio_processing="features", audio_train_record=p["audio"],
              labels_train_record=p["labels"], encoder_units_per_layer=((16,), (16, 16)), decoder_units_per_layer=(16,),
              use_ctc=True, decoding_algorithm="attention_rescoring", beam_width=10)
    exp = _construct(monkeypatch, dict(kw, ctc_decode_weight=0.3))
    assert exp._decoding_algorithm == "attention_rescoring" and exp._ctc_decode_weight == 0.3 and exp._cfg.use_ctc
    assert _construct(monkeypatch, kw)._ctc_decode_weight == 0.0            # the default: s_att alone
    assert _construct(monkeypatch, dict(kw, architecture="bimodal", video_processing="features", video_train_record=p["video"],
                                        encoder_units_per_layer=((16,), (16,))))._cfg.architecture == "bimodal"


def test_avsr_refuses_what_rescoring_does_not_cover(tmp_path):
    """Raised on the host, before any engine is built: no GPU and no data records are needed to get these answers."""
    import avsr_tf1_amd as avsr
    kw = dict(unit="character", unit_file=_unit_file(tmp_path), decoding_algorithm="attention_rescoring")
    with pytest.raises(ValueError, match="use_ctc"):
        avsr.AVSR(**kw)
    with pytest.raises(ValueError, match="use_ctc"):
        avsr.AVSR(ctc_decode_weight=0.3, **kw)
    with pytest.raises(ValueError, match="64"):
        avsr.AVSR(use_ctc=True, beam_width=65, **kw)
    with pytest.raises(ValueError, match="64"):
        avsr.AVSR(use_ctc=True, beam_width=0, **kw)
    big = "".join(chr(0x100 + i) for i in range(300))
    with pytest.raises(ValueError, match="256"):
        avsr.AVSR(use_ctc=True, **dict(kw, unit_file=_unit_file(tmp_path, big)))
    for bad in (-0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="ctc_decode_weight"):
            avsr.AVSR(use_ctc=True, ctc_decode_weight=bad, **kw)
    with pytest.raises(NotImplementedError, match="write_attention_alignment"):
        avsr.AVSR(use_ctc=True, write_attention_alignment=True, **kw)
    with pytest.raises(ValueError, match="beam_search"):                          # the language model stays on the beam
        avsr.AVSR(use_ctc=True, lm_checkpoint="nowhere", **kw)


def test_refusals_pinned_before_this_algorithm_keep_their_type_and_wording(tmp_path):
    import avsr_tf1_amd as avsr
    kw = dict(unit="character", unit_file=_unit_file(tmp_path))
    with pytest.raises(Exception, match="ctc_prefix_beam_search") as e:
        avsr.AVSR(decoding_algorithm="viterbi", **kw)
    assert "attention_rescoring" in str(e.value) and "greedy" in str(e.value) and "beam_search" in str(e.value)
    for alg in ("greedy", "ctc_prefix_beam_search"):
        with pytest.raises(ValueError, match="beam_search"):
            avsr.AVSR(use_ctc=True, ctc_decode_weight=0.3, decoding_algorithm=alg, **kw)
        with pytest.raises(ValueError, match="beam_search"):
            avsr.AVSR(use_ctc=True, lm_checkpoint="nowhere", decoding_algorithm=alg, **kw)
    with pytest.raises(ValueError, match="use_ctc"):
        avsr.AVSR(ctc_decode_weight=0.3, decoding_algorithm="beam_search", **kw)
    with pytest.raises(NotImplementedError, match="write_attention_alignment"):
        avsr.AVSR(write_attention_alignment=True, decoding_algorithm="beam_search", **kw)


def test_entry_points_reject_bad_arguments_before_any_launch():
    from avsr_tf1_amd import _lib
    lib = _lib.load()
    assert lib.avsr_abi_version() == 2
    p = 64                                          # any non-NULL address: the checks return before a launch could read it

    def logprob(logits=p, labels=p, lens=p, B=3, L=7, V=31, out=p, stride=1):
        return lib.avsr_seq_logprob(logits, labels, lens, B, L, V, out, stride, None)

    for n in ("logits", "labels", "lens", "out"):
        assert logprob(**{n: None}) == -1, n
    assert logprob(B=0) == -1 and logprob(B=-2) == -1 and logprob(L=0) == -1 and logprob(stride=0) == -1 and logprob(stride=-10) == -1
    assert logprob(V=1) == -1 and logprob(V=0) == -1
    assert logprob(V=1025) == -3                                                    # AVSR_ERR_UNSUPPORTED
    assert logprob(V=1025, out=None) == -1                                          # an argument error comes first

    def select(s_att=p, s_ctc=p, n=p, B=3, K=10, w=0.3, order=p, final=p):
        return lib.avsr_rescore_select(s_att, s_ctc, n, B, K, w, order, final, None)

    for nme in ("s_att", "s_ctc", "n", "order", "final"):
        assert select(**{nme: None}) == -1, nme
    assert select(B=0) == -1 and select(K=0) == -1 and select(K=65) == -1 and select(K=-1) == -1
    assert select(w=-0.5) == -1 and select(w=float("inf")) == -1 and select(w=float("nan")) == -1


def test_new_entry_points_are_declared_bound_and_documented():
    from avsr_tf1_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "avsr_hip.h")).read()
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    for sym in ("avsr_seq_logprob", "avsr_rescore_select"):
        assert sym in _lib.EXPORTS and ("int %s(" % sym) in hdr and sym in doc
    assert "attention_rescoring" in doc
