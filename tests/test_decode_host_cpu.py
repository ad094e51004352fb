"""The host side of the six evaluation decodes (greedy, beam search, CTC best path, forced alignment, CTC prefix beam search, attention
rescoring), the parts that need no GPU: every refusal they raise before touching the device, character for character, and the one redo
wrapper they share (model_base.EvalMixin._redo_if_flagged).  Models are bare objects with a configuration and no engine."""
import types

import pytest
import torch

from avsr_tf1_amd.config import ModelConfig
from avsr_tf1_amd.model import Seq2SeqModel

NAN, INF = float("nan"), float("inf")


def _model(**cfg):
    m = object.__new__(Seq2SeqModel)
    m.cfg, m.dev = ModelConfig(**cfg), torch.device("cpu")
    return m


def _batch():
    return types.SimpleNamespace(audio=torch.zeros(2, 5, 3), video=None, labels=torch.zeros(2, 4, dtype=torch.int32))


def _lm(**over):
    """What _check_lm and the prefix search's shape refusal read of a language model: its configuration and `onehot`."""
    kw = dict(architecture="lm", cell_type="lstm", vocab_size=31, go_id=30, eos_id=29, decoder_units=(256,), embedding_size=128)
    kw.update(over)
    return types.SimpleNamespace(cfg=types.SimpleNamespace(**kw), onehot=None)


def _ngram(**over):
    g = dict(V=31, go_id=30, eos_id=29, n_nodes=10, n_arcs=20)
    g.update(over)
    return g


CTC, LM = dict(use_ctc=True), dict(architecture="lm", video_units=None, audio_units=None)
prefix = lambda beam_width=4, max_steps=None, **kw: lambda m: m._ctc_prefix_beam_search(_batch(), beam_width, max_steps, False, **kw)
rescore = lambda beam_width=4, max_steps=None, ctc_weight=0.0: lambda m: m._attention_rescoring(_batch(), beam_width, max_steps, ctc_weight, False)
beam = lambda **kw: lambda m: m._beam_search_decode(_batch(), **kw)

# (case, configuration, call, exception, the text the decode raised before its shared steps were gathered into helpers)
REFUSALS = [
    ("best_path/no_ctc", {}, lambda m: m._ctc_best_path(_batch()), ValueError, "ctc_best_path needs a model built with use_ctc=True"),
    ("align/no_ctc", {}, lambda m: m._ctc_align(_batch(), None), ValueError, "ctc_align needs a model built with use_ctc=True"),
    ("align/lm", LM, lambda m: m._ctc_align(_batch(), None), ValueError,
     "ctc_align: architecture='lm' has no encoder, so no CTC head to align on"),
    ("align/targets", CTC, lambda m: m._ctc_align(_batch(), [[1, 2]]), ValueError,
     "ctc_align: targets must hold one id list per utterance (got 1 lists for a batch of 2)"),
    ("align/long", CTC, lambda m: m._ctc_align(_batch(), [[1] * 513, [2]]), ValueError,
     "ctc_align: avsr_ctc_align covers targets of up to 512 labels (got 513)"),
    ("prefix/no_ctc", {}, prefix(), ValueError, "ctc_prefix_beam_search needs a model built with use_ctc=True"),
    ("prefix/width0", CTC, prefix(beam_width=0), ValueError, "ctc_prefix_beam_search: beam_width and max_steps must be positive (got 0, 150)"),
    ("prefix/steps0", CTC, prefix(max_steps=0), ValueError, "ctc_prefix_beam_search: beam_width and max_steps must be positive (got 4, 0)"),
    ("prefix/width-3", CTC, prefix(beam_width=-3, max_steps=-1), ValueError,
     "ctc_prefix_beam_search: beam_width and max_steps must be positive (got -3, -1)"),
    ("prefix/width65", CTC, prefix(beam_width=65), ValueError,
     "ctc_prefix_beam_search: avsr_ctc_prefix_search covers vocabularies of up to 256 symbols, beam widths of up to 64 and label sequences "
     "of up to 512 (got 31, 65, 150)"),
    ("prefix/steps513", CTC, prefix(max_steps=513), ValueError,
     "ctc_prefix_beam_search: avsr_ctc_prefix_search covers vocabularies of up to 256 symbols, beam widths of up to 64 and label sequences "
     "of up to 512 (got 31, 4, 513)"),
    ("prefix/lm_and_ngram", CTC, prefix(lm=_lm(), ngram=_ngram()), ValueError,
     "ctc_prefix_beam_search takes one language model: lm (an avsr.LM network) or ngram (back-off tables), not both"),
    ("prefix/lm_weight_nan", CTC, prefix(ngram=_ngram(), lm_weight=NAN), ValueError,
     "ctc_prefix_beam_search: lm_weight must be a finite number >= 0 (got nan)"),
    ("prefix/lm_weight_neg", CTC, prefix(ngram=_ngram(), lm_weight=-0.5), ValueError,
     "ctc_prefix_beam_search: lm_weight must be a finite number >= 0 (got -0.5)"),
    ("prefix/lm_weight_neg_int", CTC, prefix(lm=_lm(), lm_weight=-1), ValueError,
     "ctc_prefix_beam_search: lm_weight must be a finite number >= 0 (got -1.0)"),
    ("prefix/lm_weight_inf", CTC, prefix(lm=_lm(), lm_weight=INF), ValueError,
     "ctc_prefix_beam_search: lm_weight must be a finite number >= 0 (got inf)"),
    ("prefix/bonus_nan", CTC, prefix(ngram=_ngram(), length_bonus=NAN), ValueError,
     "ctc_prefix_beam_search: length_bonus must be finite (got nan)"),
    ("prefix/bonus_inf", CTC, prefix(lm=_lm(), length_bonus=-INF), ValueError,
     "ctc_prefix_beam_search: length_bonus must be finite (got -inf)"),
    ("prefix/ngram_vocab", CTC, prefix(ngram=_ngram(V=40, eos_id=39)), ValueError,
     "ctc_prefix_beam_search: the n-gram tables were compiled for V = 40, GO = 30, EOS = 39; the model has 31, 30, 29"),
    ("prefix/ngram_width17", CTC, prefix(beam_width=17, ngram=_ngram()), ValueError,
     "ctc_prefix_beam_search: with an n-gram avsr_ctc_prefix_search_ngram covers beam widths of up to 16 (vocabularies of up to 256 "
     "symbols, label sequences of up to 512) and automata of up to 16777216 nodes and 67108864 arcs (got beam width 17, 31 symbols, "
     "150 labels, 10 nodes, 20 arcs)"),
    ("prefix/lm_width17", CTC, prefix(beam_width=17, lm=_lm()), ValueError,
     "ctc_prefix_beam_search: with a language model avsr_ctc_prefix_search_lm covers beam widths of up to 16 (vocabularies of up to 256 "
     "symbols, label sequences of up to 512) and LSTM models of up to 4 equal layers (got beam width 17, 31 symbols, 150 labels, 1 layers "
     "of 256 units)"),
    ("prefix/check_lm", CTC, prefix(lm=object()), ValueError, "beam search: lm must be a Seq2SeqModel with architecture='lm'"),
    ("rescore/lm", LM, rescore(), ValueError,
     "attention_rescoring: architecture='lm' has no encoder, so no CTC head whose n-best could be rescored"),
    ("rescore/no_ctc", {}, rescore(), ValueError,
     "attention_rescoring needs a model built with use_ctc=True: the hypotheses are the CTC head's n-best"),
    ("rescore/weight_nan", CTC, rescore(ctc_weight=NAN), ValueError, "attention_rescoring: ctc_weight must be a finite number >= 0 (got nan)"),
    ("rescore/weight_neg", CTC, rescore(ctc_weight=-0.25), ValueError,
     "attention_rescoring: ctc_weight must be a finite number >= 0 (got -0.25)"),
    ("rescore/weight_neg_int", CTC, rescore(ctc_weight=-1), ValueError, "attention_rescoring: ctc_weight must be a finite number >= 0 (got -1)"),
    ("rescore/weight_inf", CTC, rescore(ctc_weight=INF), ValueError, "attention_rescoring: ctc_weight must be a finite number >= 0 (got inf)"),
    ("rescore/width0", CTC, rescore(beam_width=0), ValueError, "attention_rescoring: beam_width and max_steps must be positive (got 0, 150)"),
    ("rescore/steps0", CTC, rescore(max_steps=0), ValueError, "attention_rescoring: beam_width and max_steps must be positive (got 4, 0)"),
    ("rescore/width65", CTC, rescore(beam_width=65), ValueError,
     "attention_rescoring: avsr_ctc_prefix_search covers vocabularies of up to 256 symbols, beam widths of up to 64 and label sequences "
     "of up to 512 (got 31, 65, 150)"),
    ("beam/weight_nan", CTC, beam(ctc_weight=NAN), ValueError, "beam search: ctc_weight must be a finite number >= 0 (got nan)"),
    ("beam/weight_neg", CTC, beam(ctc_weight=-0.3), ValueError, "beam search: ctc_weight must be a finite number >= 0 (got -0.3)"),
    ("beam/weight_neg_int", CTC, beam(ctc_weight=-1), ValueError, "beam search: ctc_weight must be a finite number >= 0 (got -1.0)"),
    ("beam/weight_inf", CTC, beam(ctc_weight=INF), ValueError, "beam search: ctc_weight must be a finite number >= 0 (got inf)"),
    ("beam/no_ctc", {}, beam(ctc_weight=0.3), ValueError, "beam search: ctc_weight needs a model built with use_ctc=True"),
    ("beam/width0", {}, beam(beam_width=0), ValueError,
     "beam search: beam_width must be in 1..64 with beam_width * vocabulary <= 1024 (got 0 x 31); the reference's default width 10 fits "
     "every shipped unit list"),
    ("beam/width65", dict(vocab_size=8, go_id=7, eos_id=6), beam(beam_width=65), ValueError,
     "beam search: beam_width must be in 1..64 with beam_width * vocabulary <= 1024 (got 65 x 8); the reference's default width 10 fits "
     "every shipped unit list"),
    ("beam/width_x_vocab", {}, beam(beam_width=34), ValueError,
     "beam search: beam_width must be in 1..64 with beam_width * vocabulary <= 1024 (got 34 x 31); the reference's default width 10 fits "
     "every shipped unit list"),
    ("greedy/lm", {}, lambda m: m.greedy_decode(_batch(), lm=_lm()), ValueError,
     "greedy_decode: language-model fusion is defined on the beam (beam_search_decode(lm=...))"),
    ("greedy/ctc_weight", {}, lambda m: m.greedy_decode(_batch(), ctc_weight=0.3), ValueError,
     "greedy_decode: joint CTC / attention scoring is defined on the beam (beam_search_decode(ctc_weight=...))"),
    ("check_lm/not_an_lm", {}, beam(lm=_lm(architecture="unimodal")), ValueError,
     "beam search: lm must be a Seq2SeqModel with architecture='lm'"),
    ("check_lm/gru", {}, beam(lm=_lm(cell_type="gru")), NotImplementedError,
     "beam search: only LSTM language models are fused (cell_type='gru')"),
    ("check_lm/vocabulary", {}, beam(lm=_lm(vocab_size=40, eos_id=39)), ValueError,
     "beam search: the language model's vocabulary / GO / EOS (40, 30, 39) differ from the recogniser's (31, 30, 29)"),
    ("check_lm/layers", {}, beam(lm=_lm(decoder_units=(64,) * 5)), NotImplementedError, "beam search: language models of up to 4 layers"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=lambda c: c[0])
def test_refusals_before_the_device_keep_their_text(case):
    _name, cfg, call, exc, text = case
    with pytest.raises(exc) as e:
        call(_model(**cfg))
    assert type(e.value) is exc and str(e.value) == text


def _flags(*answers):
    """A check_persistent that gives `answers` in turn, and the list of its calls."""
    seen, it = [], iter(answers)

    def check_persistent(*a, **kw):
        seen.append((a, kw))
        return next(it)
    return check_persistent, seen


def test_redo_helper_runs_twice_with_the_same_arguments_when_flagged():
    m = _model()
    m.check_persistent, seen = _flags(True, False)
    calls = []

    def fn(*a, **kw):
        calls.append((a, kw))
        return len(calls)
    assert m._redo_if_flagged(fn, 1, "x", k=[2]) == 2                     # the second result
    assert calls == [((1, "x"), {"k": [2]})] * 2 and len(seen) == 1       # (the flag is read once: the redo is not checked again)
    assert m._redo_if_flagged(fn, 3) == 3 and len(calls) == 3 and len(seen) == 2


PUBLIC = [
    ("greedy_decode", "_greedy_decode", lambda m, b: m.greedy_decode(b, max_steps=7), ((), dict(max_steps=7))),
    ("beam_search_decode", "_beam_search_decode", lambda m, b: m.beam_search_decode(b, 5, lm="LM", ctc_weight=0.3),
     ((5,), dict(lm="LM", ctc_weight=0.3))),
    ("ctc_best_path", "_ctc_best_path", lambda m, b: m.ctc_best_path(b), ((), {})),
    ("ctc_align", "_ctc_align", lambda m, b: m.ctc_align(b, [[1], [2]]), (([[1], [2]],), {})),
    ("ctc_prefix_beam_search", "_ctc_prefix_beam_search", lambda m, b: m.ctc_prefix_beam_search(b, 4, 9, True, "LM", 0.5, 0.1, None),
     ((4, 9, True, "LM", 0.5, 0.1, None), {})),
    ("attention_rescoring", "_attention_rescoring", lambda m, b: m.attention_rescoring(b, 4, 9, 0.2, True), ((4, 9, 0.2, True), {})),
]


@pytest.mark.parametrize("flagged", [False, True])
@pytest.mark.parametrize("case", PUBLIC, ids=lambda c: c[0])
def test_public_decodes_reach_their_private_form_through_the_redo_helper(case, flagged, monkeypatch):
    _name, private, call, (args, kw) = case
    m, b = _model(use_ctc=True), _batch()
    m.check_persistent, seen = _flags(*([True, False] if flagged else [False]))
    calls, through = [], []

    def stub(*a, **k):
        calls.append((a, k))
        return "pass %d" % len(calls)
    monkeypatch.setattr(m, private, stub, raising=True)
    redo = Seq2SeqModel._redo_if_flagged
    monkeypatch.setattr(Seq2SeqModel, "_redo_if_flagged", lambda self, fn, *a, **k: (through.append(fn), redo(self, fn, *a, **k))[1])
    assert call(m, b) == ("pass 2" if flagged else "pass 1")
    assert through == [stub] and len(seen) == 1                           # check_persistent is consulted once per public call
    assert calls == [((b,) + args, kw)] * (2 if flagged else 1)
