"""fp64 reference of beam search with a shallow-fusion language model (include/avsr_hip.h avsr_beam_lm): the oracle's own beam loop
(oracle.beam_search_decode) with one more score term.  Everything of the step is the oracle's -- `_Model.step`, `_embedding`,
`beam_candidates`, `beam_advance`, `gather_tree` -- and the language model advances with the oracle's `lstm_cell` from the zero state:

    step_lp[k, v] = log_softmax(logits_am[k])[v] + lm_weight * log_softmax(logits_lm[k])[v]

`beam_candidates` then replaces a finished beam's row by {EOS: 0, else: float32 min}: no language-model term reaches it.  lm_weight == 0
leaves the acoustic term alone (as the kernel branches on the weight), so the result IS oracle.beam_search_decode's.
`follow=` is the oracle's test aid: score every step from the state the followed implementation's own branch leads to."""
import numpy as np
import torch

from oracle import avsr_oracle as O


def lm_zero_state(lcfg, n, dtype=torch.float64):
    return [(torch.zeros(n, H, dtype=dtype), torch.zeros(n, H, dtype=dtype)) for H in lcfg.decoder_units]


def lm_step(P, lcfg, tok, state):
    """One step of avsr.LM's evaluate graph: tok [n] int64 -> (log_softmax [n, V], new state).  P: torch tensors in TF layout."""
    x = O._embedding(P, lcfg)[tok]
    new = []
    for j, (c, h) in enumerate(state):
        c, h = O.lstm_cell(x, c, h, P["dec/l%d/kernel" % j], P["dec/l%d/bias" % j])
        new.append((c, h))
        x = h
    logits = x @ P["dec/out/kernel"] + P["dec/out/bias"]
    return torch.log_softmax(logits, dim=-1), new


def lm_init_params(lcfg, seed=31, scale=3.0, eos_bias=1.5):
    """Random language-model weights with a SHARP output layer (the term must be able to change a selection) that leans towards EOS
    (a search over random weights must still end)."""
    W = O.init_params(lcfg, seed=seed)
    rng = np.random.default_rng(seed + 1)
    for k in W:
        if k.endswith("bias"):
            W[k] = (rng.standard_normal(W[k].shape) * 0.3).astype(np.float32)
    W["dec/out/kernel"] = (W["dec/out/kernel"] * scale).astype(np.float32)
    W["dec/out/bias"][lcfg.eos_id] += eos_bias
    return W


def fused_candidates(logp, finished, lengths, am_lp, lm_lp, lm_weight, w, eos):
    """oracle.beam_candidates on the fused step log-probabilities [B, K, V] (the whole scoring rule)."""
    step_lp = am_lp if lm_weight == 0.0 else am_lp + lm_weight * lm_lp
    return O.beam_candidates(logp, finished, lengths, step_lp, w, eos)


@torch.no_grad()
def beam_search_decode_lm(P_np, cfg, batch, lm_np, lcfg, lm_weight, beam_width=10, length_penalty_weight=None, max_steps=None,
                          dtype=torch.float64, follow=None):
    """Returns ids [B, T, K], logp [B, K], lengths [B, K], trace (as oracle.beam_search_decode(return_trace=True))."""
    P, PL = O.to_torch(P_np, dtype), O.to_torch(lm_np, dtype)
    m = O._Model(P, cfg, batch, False, dtype)
    B, K, V, eos = m.B, beam_width, cfg.vocab_size, cfg.eos_id
    assert (lcfg.vocab_size, lcfg.go_id, lcfg.eos_id) == (V, cfg.go_id, eos)
    w = length_penalty_weight if length_penalty_weight is not None else (0.5 if cfg.architecture == "bimodal" else 0.6)
    max_steps = cfg.max_label_length if max_steps is None else max_steps
    tile = lambda t: t.repeat_interleave(K, dim=0)
    for mech in m.mechs:
        mech.values, mech.keys, mech.mask = tile(mech.values), tile(mech.keys), tile(mech.mask)
    state = tuple(tile(s) for s in m.init_state)
    lm_state = lm_zero_state(lcfg, B * K, dtype)
    att = torch.zeros(B * K, m.att_dim, dtype=dtype)
    tok = torch.full((B * K,), cfg.go_id, dtype=torch.int64)
    logp = torch.full((B, K), -float("inf"), dtype=dtype)
    logp[:, 0] = 0.0
    finished = torch.zeros(B, K, dtype=torch.bool)
    lengths = torch.zeros(B, K, dtype=torch.int64)
    step_ids, parent_ids, step_gaps = [], [], []
    f_dev, f_same, f_distinct, f_short = [], [], [], False
    for t in range(max_steps):
        out, state, att, _ = m.step(O._embedding(P, cfg)[tok], state, att, t)
        step_lp = torch.log_softmax(m.logits(out), dim=-1)
        lm_lp, lm_state = lm_step(PL, lcfg, tok, lm_state)
        total, scores = fused_candidates(logp, finished, lengths, step_lp.reshape(B, K, V), lm_lp.reshape(B, K, V), lm_weight, w, eos)
        order_all = torch.argsort(scores, dim=1, descending=True, stable=True)
        order = order_all[:, :K]
        top = torch.gather(scores, 1, order_all[:, :K + 1])
        gap = top[:, :-1] - top[:, 1:]
        gap = torch.where((top[:, :-1] == top[:, 1:]) | torch.isnan(gap), torch.full_like(gap, float("inf")), gap)
        step_gaps.append(gap.min(dim=1).values.numpy())
        if follow is not None:
            if t >= follow[0].shape[0]:
                f_short = True
                break
            eng = torch.as_tensor(follow[1][t].astype(np.int64)) * V + torch.as_tensor(follow[0][t].astype(np.int64))
            s_eng, s_ref = torch.gather(scores, 1, eng), torch.gather(scores, 1, order)
            both_inf = torch.isinf(s_eng) & torch.isinf(s_ref) & (s_eng == s_ref)
            dev = torch.where(both_inf, torch.zeros_like(s_ref), (s_eng - s_ref).abs() / torch.clamp(s_ref.abs(), min=1.0))
            dev = torch.where(torch.isnan(dev), torch.full_like(dev, float("inf")), dev)
            f_dev.append(dev.max(dim=1).values.numpy())
            f_same.append((eng == order).all(dim=1).numpy())
            srt = torch.sort(eng, dim=1).values
            f_distinct.append(((srt[:, 1:] != srt[:, :-1]).all(dim=1) if K > 1 else torch.ones(B, dtype=torch.bool)).numpy())
            order = eng
        word, parent = order % V, order // V
        logp, finished, lengths = O.beam_advance(total, finished, lengths, order, V, eos)
        rows = (torch.arange(B)[:, None] * K + parent).reshape(-1)
        state = tuple(s[rows] for s in state)
        lm_state = [(c[rows], h[rows]) for c, h in lm_state]
        att = att[rows]
        tok = word.reshape(-1)
        step_ids.append(word.numpy().astype(np.int32))
        parent_ids.append(parent.numpy().astype(np.int32))
        if bool(finished.all()):
            break
    sid, pid = np.stack(step_ids), np.stack(parent_ids)
    beams = O.gather_tree(sid, pid, lengths.max(dim=1).values.numpy(), eos)
    ids = np.ascontiguousarray(beams.transpose(1, 0, 2))
    tr = dict(step_ids=sid, parent_ids=pid, gaps=np.stack(step_gaps)[:sid.shape[0]], finished=finished.numpy())
    if follow is not None:
        tr.update(follow_dev=np.stack(f_dev), follow_same=np.stack(f_same), follow_distinct=np.stack(f_distinct), follow_short=f_short)
    return ids, logp.numpy(), lengths.numpy(), tr


# ---- the small search cases shared by tests/test_beam_lm_cpu.py and tests/test_gpu_beam_lm.py --------------------------------------
_LUONG, _BAHDANAU = (("scaled_luong",), ("scaled_luong",)), (("bahdanau",), ("bahdanau",))
ARCHS = {"c1_audio_uni_luong": dict(architecture="unimodal", encoder_type="unidirectional", video_units=None, audio_units=(16,), attention_type=_LUONG),
         "c2_audio_bi_bahdanau": dict(architecture="unimodal", encoder_type="bidirectional", video_units=None, audio_units=(16, 16),
                                      attention_type=_BAHDANAU),
         "c4_bimodal_uni": dict(architecture="bimodal", encoder_type="unidirectional", video_units=(16,), audio_units=(16, 16),
                                attention_type=_LUONG, regress_aus=True),
         "c5_av_align": dict(architecture="av_align", encoder_type="unidirectional", video_units=(16,), audio_units=(16, 16), attention_type=_LUONG,
                             regress_aus=True)}
LMS = {"1x10": dict(decoder_units=(10,), embedding_size=6),                    # 12 units, 8 inputs inside the engine
       "2x10_onehot": dict(decoder_units=(10, 10), embedding_size=0)}          # two layers, one-hot inputs (V = 31 -> 32 inside)
MAX_STEPS = 11            # not a multiple of the check_every the GPU test uses: a chunk runs past the end of the search
_cases = {}


def _model_config(ocfg):
    import dataclasses
    from avsr_tf1_amd.config import ModelConfig
    return ModelConfig(**{f.name: getattr(ocfg, f.name) for f in dataclasses.fields(ModelConfig) if hasattr(ocfg, f.name)})


def _recogniser(case):
    """Random recogniser one train step off its initial point with a SHARP output layer that leans towards EOS: with the near-uniform
    distributions of untouched random weights almost every step would be a near-tie, and the search would not end."""
    ocfg = O.OracleConfig(decoder_units=(16,), embedding_size=16, video_feat=12, audio_feat=20, **ARCHS[case])
    W = O.init_params(ocfg, seed=2001)
    rng = np.random.default_rng(7)
    for k in W:
        if k.endswith(("bias", "/b", "beta")):
            W[k] = (rng.standard_normal(W[k].shape) * 0.1).astype(np.float32)
        if k.endswith("gamma"):
            W[k] = (1.0 + rng.standard_normal(W[k].shape) * 0.1).astype(np.float32)
        if k.endswith("/g"):
            W[k] = (W[k] * 1.3).astype(np.float32)
    batch = O.synthetic_batch(ocfg, B=3, T_a=12, T_v=5, L=7, ragged=True, seed=1000)
    W2 = {k: v.copy() for k, v in O.train_step(W, None, ocfg, batch)["params"].items()}
    rng = np.random.default_rng(5)
    W2["dec/out/kernel"] = (W2["dec/out/kernel"] * 10.0).astype(np.float32)
    W2["dec/out/bias"] = rng.standard_normal(W2["dec/out/bias"].shape).astype(np.float32)
    W2["dec/out/bias"][ocfg.eos_id] += 4.0
    return ocfg, W2, batch


def search_case(case, lm="1x10"):
    """(ocfg, mcfg, W, batch, lcfg, lmcfg, WL): B = 3 of unequal lengths, T_a = 12, T_v = 5, decoder width 16 and the language model
    LMS[lm].  Built once per (case, lm) and shared; nothing in it is modified afterwards."""
    if (case, lm) not in _cases:
        if (case, None) not in _cases:
            _cases[(case, None)] = _recogniser(case)
        ocfg, W2, batch = _cases[(case, None)]
        lcfg = O.OracleConfig(architecture="lm", video_units=None, audio_units=None, warmup_steps=0, **LMS[lm])
        _cases[(case, lm)] = (ocfg, _model_config(ocfg), W2, batch, lcfg, _model_config(lcfg), lm_init_params(lcfg))
    return _cases[(case, lm)]
