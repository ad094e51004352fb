"""fp64 reference of beam search with a shallow-fusion back-off n-gram (include/avsr_hip.h avsr_beam_ngram).

The search is ref_beam_ctc.beam_search_decode_ctc's loop, `follow=` included; in place of the LSTM's log_softmax it reads

    lam(. | GO, g_k)      from a ref_ngram.NGramRef (the textbook rule over dictionaries, float64) over each row's OWN label history

so the reference knows nothing of nodes, transitions or the compiled automaton.  The CTC term is optional, through ref_beam_ctc's `step`.
    step_lp[k, v] = log_softmax(logits_am[k])[v] + lm_weight * lam(v | GO, g_k)  (+ ctc_weight * term)
`beam_candidates` then replaces a finished beam's row by {EOS: 0, else: float32 min}: no term reaches it.  lm_weight == 0 leaves the
acoustic term alone (as the kernel branches on the weight), so the result IS oracle.beam_search_decode's.

The search cases come in two setups: ref_beam_lm.search_case as it is (MAX_STEPS 11: searches end after a few steps, and a chunk of the
engine's is queued past the end), and the LONG setup -- the same recogniser with a copy of dec/out/bias lowered by 2.0 at EOS and
max_steps = 9 -- in which the histories grow longer than the order, so that the state really is the last N-1 symbols.
`host_step` / `host_node` / `host_rows` restate the device step on the compiled tables with ngram.walk (float32, the kernel's order)."""
import numpy as np
import torch

import ref_beam_ctc as RC
import ref_beam_lm as RL
import ref_ngram as RN
from oracle import avsr_oracle as O

ARCHS = RL.ARCHS
ORDERS = RN.ORDERS
WEIGHTS = (0.3, 1.0)
KS = (1, 3, 10)
MAX_STEPS = RL.MAX_STEPS          # the unmodified setup
LONG_STEPS = 9
LONG_EOS_SHIFT = -2.0
V = 31                            # the recogniser's vocabulary: 28 characters + MASK, EOS, GO
_long = {}


def long_case(case):
    """(ocfg, mcfg, W, batch) of the long setup; built once per case and shared, ref_beam_lm's weights are not touched."""
    if case not in _long:
        ocfg, mcfg, W, batch = RL.search_case(case)[:4]
        W = dict(W)
        W["dec/out/bias"] = W["dec/out/bias"].copy()
        W["dec/out/bias"][ocfg.eos_id] += np.float32(LONG_EOS_SHIFT)
        _long[case] = (ocfg, mcfg, W, batch)
    return _long[case]


def plain_case(case):
    return RL.search_case(case)[:4]


def ctc_case(case):
    return RC.search_case(case)[:4]


def model(order, V=V):
    return RN.shared_model(order, V)


@torch.no_grad()
def beam_search_decode_ngram(P_np, cfg, batch, ref, lm_weight, ctc_weight=0.0, beam_width=10, length_penalty_weight=None, max_steps=None,
                             follow=None):
    """ref: a ref_ngram.NGramRef.  Returns ids [B, T, K], logp [B, K], lengths [B, K], trace (as ref_beam_ctc.beam_search_decode_ctc;
    trace['cuts'][t] holds the score gap between the K-th and the (K+1)-th candidate of every utterance,
    trace['hists'][t] the label history of every row at step t, trace['lams'][t] the rows lam(. | GO, history) [B * K, V])."""
    dtype = torch.float64
    P = O.to_torch(P_np, dtype)
    m = O._Model(P, cfg, batch, False, dtype)
    B, K, V, eos = m.B, beam_width, cfg.vocab_size, cfg.eos_id
    assert (ref.V, ref.go, ref.eos) == (V, cfg.go_id, eos)
    w = length_penalty_weight if length_penalty_weight is not None else (0.5 if cfg.architecture == "bimodal" else 0.6)
    max_steps = cfg.max_label_length if max_steps is None else max_steps
    if ctc_weight != 0.0:
        z, Tb_u = RC.head_logits(P, m, cfg)
        y = np.repeat(RC.log_softmax(z), K, axis=0)
        Tb = np.repeat(Tb_u, K)
        cst = RC.empty_state(y, Tb)
    tile = lambda t: t.repeat_interleave(K, dim=0)
    for mech in m.mechs:
        mech.values, mech.keys, mech.mask = tile(mech.values), tile(mech.keys), tile(mech.mask)
    state = tuple(tile(s) for s in m.init_state)
    hist = [() for _ in range(B * K)]
    att = torch.zeros(B * K, m.att_dim, dtype=dtype)
    tok = torch.full((B * K,), cfg.go_id, dtype=torch.int64)
    logp = torch.full((B, K), -float("inf"), dtype=dtype)
    logp[:, 0] = 0.0
    finished = torch.zeros(B, K, dtype=torch.bool)
    lengths = torch.zeros(B, K, dtype=torch.int64)
    rows = torch.arange(B * K)
    step_ids, parent_ids, step_gaps, step_cuts, hists, lams = [], [], [], [], [], []
    f_dev, f_same, f_distinct, f_short = [], [], [], False
    for t in range(max_steps):
        out, state, att, _ = m.step(O._embedding(P, cfg)[tok], state, att, t)
        step_lp = torch.log_softmax(m.logits(out), dim=-1)
        lam = np.stack([ref.lam(g) for g in hist]).astype(np.float64)
        hists.append(list(hist))
        lams.append(lam)
        if lm_weight != 0.0:
            step_lp = step_lp + lm_weight * torch.as_tensor(lam)
        if ctc_weight != 0.0:
            cst, tm = RC.step(y, Tb, cst, tok.numpy(), rows.numpy(), finished.reshape(-1).numpy(), t, eos)
            step_lp = step_lp + ctc_weight * torch.as_tensor(tm.astype(np.float64))
        total, scores = O.beam_candidates(logp, finished, lengths, step_lp.reshape(B, K, V), w, eos)
        order_all = torch.argsort(scores, dim=1, descending=True, stable=True)
        order = order_all[:, :K]
        top = torch.gather(scores, 1, order_all[:, :K + 1])
        gap = top[:, :-1] - top[:, 1:]
        gap = torch.where((top[:, :-1] == top[:, 1:]) | torch.isnan(gap), torch.full_like(gap, float("inf")), gap)
        step_gaps.append(gap.min(dim=1).values.numpy())
        step_cuts.append(gap[:, K - 1].numpy())                              # the K-th candidate against the (K+1)-th: the cut of the selection
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
        att = att[rows]
        tok = word.reshape(-1)
        hist = [hist[int(r)] + (int(c),) for r, c in zip(rows, tok)]
        step_ids.append(word.numpy().astype(np.int32))
        parent_ids.append(parent.numpy().astype(np.int32))
        if bool(finished.all()):
            break
    sid, pid = np.stack(step_ids), np.stack(parent_ids)
    beams = O.gather_tree(sid, pid, lengths.max(dim=1).values.numpy(), eos)
    ids = np.ascontiguousarray(beams.transpose(1, 0, 2))
    tr = dict(step_ids=sid, parent_ids=pid, gaps=np.stack(step_gaps)[:sid.shape[0]], cuts=np.stack(step_cuts)[:sid.shape[0]],
              finished=finished.numpy(), hists=hists, lams=lams)
    if follow is not None:
        tr.update(follow_dev=np.stack(f_dev), follow_same=np.stack(f_same), follow_distinct=np.stack(f_distinct), follow_short=f_short)
    return ids, logp.numpy(), lengths.numpy(), tr


# ---- the device step restated on the compiled tables (ngram.walk: float32, the kernel's additions in the kernel's order) -------------
def host_transition(tables, node, c):
    from avsr_tf1_amd import ngram
    return int(tables["next"][ngram.walk(tables, int(node), int(c))[1]])


def host_node(tables, g):
    """The node of the label history g: `start`, moved along every symbol."""
    n = int(tables["start"])
    for c in g:
        n = host_transition(tables, n, c)
    return n


def host_step(tables, nodes, tok, parent_rows, step):
    """One avsr_beam_ngram_step on the host: the new nodes [R] of the rows."""
    if step == 0:
        return np.full(len(tok), int(tables["start"]), np.int32)
    return np.array([host_transition(tables, nodes[p], c) for p, c in zip(parent_rows, tok)], np.int32)


_rows = {}


def host_rows(tables, nodes):
    """lam(. | node) [len(nodes), V] float32 by ngram.walk (memoised per table object and node)."""
    from avsr_tf1_amd import ngram
    memo = _rows.setdefault(id(tables), {})
    V = int(tables["V"])
    for n in set(int(x) for x in nodes):
        if n not in memo:
            memo[n] = np.array([ngram.walk(tables, n, c)[0] for c in range(V)], np.float32)
    return np.stack([memo[int(n)] for n in nodes])
