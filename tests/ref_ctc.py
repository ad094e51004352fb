"""CPU references for the CTC auxiliary loss (use_ctc), fp64, none of it written here as a recursion: the loss is
torch.nn.functional.ctc_loss, composed with the oracle's train graph WITHOUT touching oracle/ -- `oracle.forward_train` returns the
model object whose `enc[stream].outputs` is still attached to the autograd graph, so the head and the CTC term are added here and the
sum is differentiated.

Definition: head z = outputs @ kernel + bias over V + 1 classes, the blank is class V (the last);
target of utterance b = labels[b, :U_b], U_b = max(min(labels_len[b], L) - 1, 0) (the label row without its EOS);
T_b = min(len[b], T); an utterance without a valid alignment contributes 0 (zero_infinity); the term is
sum_b nll_b / sum_b min(labels_len[b], L), the sequence loss's own normaliser."""
import numpy as np
import torch
import torch.nn.functional as F


def head_names(stream):
    return f"{stream}/ctc/kernel", f"{stream}/ctc/bias"


def ctc_stream(cfg):
    return "audio" if cfg.audio_units is not None else "video"


def add_head(W, ocfg, stream, seed=11):
    """A copy of the weight dict with the two head variables (glorot kernel, small non-zero bias so that its gradient path is live)."""
    D = ocfg.memory_depth(stream)
    C = ocfg.vocab_size + 1
    rng = np.random.default_rng(seed)
    lim = np.sqrt(6.0 / (D + C))
    W = dict(W)
    kn, bn = head_names(stream)
    W[kn] = rng.uniform(-lim, lim, (D, C)).astype(np.float32)
    W[bn] = (rng.standard_normal(C) * 0.1).astype(np.float32)
    return W


def targets(labels, labels_len):
    labels, labels_len = np.asarray(labels), np.asarray(labels_len)
    L = labels.shape[1]
    return np.maximum(np.minimum(labels_len, L) - 1, 0).astype(np.int64)


def ctc_nll(z, labels, labels_len, in_len, blank):
    """z [B, T, C] fp64 tensor (may require grad) -> (nll [B] with zero_infinity, U [B], T_b [B])."""
    B, T, C = z.shape
    U = torch.as_tensor(targets(labels, labels_len))
    Tb = torch.clamp(torch.tensor(np.array(in_len), dtype=torch.int64), 0, T)
    logp = torch.log_softmax(z, dim=-1).transpose(0, 1)            # [T, B, C]
    tgt = torch.tensor(np.array(labels), dtype=torch.int64)
    nll = F.ctc_loss(logp, tgt, Tb, U, blank=blank, reduction="none", zero_infinity=True)
    return nll, U, Tb


def feasible(labels, labels_len, in_len, T):
    """status of the kernel: 1 where a valid alignment exists (T_b >= U_b + adjacent equal pairs, T_b >= 1)."""
    labels = np.asarray(labels)
    U = targets(labels, labels_len)
    Tb = np.clip(np.asarray(in_len), 0, T)
    out = np.zeros(len(U), np.int32)
    for b in range(len(U)):
        rep = int(np.sum(labels[b, 1:U[b]] == labels[b, :max(U[b] - 1, 0)]))
        out[b] = int(Tb[b] >= 1 and Tb[b] >= U[b] + rep)
    return out


def kernel_reference(z, labels, labels_len, in_len, denom, weight=1.0):
    """What avsr_ctc_loss returns, in fp64: dict(nll, status, utt_loss, dz) for logits z [B, T, C] (numpy), blank = C - 1."""
    zt = torch.tensor(np.asarray(z, dtype=np.float64), requires_grad=True)
    nll, _U, _Tb = ctc_nll(zt, labels, labels_len, in_len, zt.shape[-1] - 1)
    total = weight * nll.sum() / float(denom)
    dz, = torch.autograd.grad(total, zt)
    return dict(nll=nll.detach().numpy(), status=feasible(labels, labels_len, in_len, zt.shape[1]),
                utt_loss=(weight * nll / float(denom)).detach().numpy(), dz=dz.numpy())


def ctc_reference(W, ocfg, batch, stream, weight, seed=0):
    """One train-graph forward + backward of the oracle with the CTC term added.  W holds the two head variables (add_head).
    Returns dict(loss, base_loss, ctc, nll, logits, grads, global_norm, z)."""
    from oracle import avsr_oracle as O
    P = O.to_torch(W, torch.float64, requires_grad=True)
    logits, m = O.forward_train(P, ocfg, batch, torch.float64, seed=seed)
    base, _seq = O.loss_fn(P, ocfg, batch, logits, m)
    kn, bn = head_names(stream)
    z = m.enc[stream].outputs @ P[kn] + P[bn]
    lens = batch.audio_len if stream == "audio" else batch.video_len
    nll, _U, _Tb = ctc_nll(z, batch.labels, batch.labels_len, lens, ocfg.vocab_size)
    L = batch.labels.shape[1]
    denom = float(np.minimum(np.asarray(batch.labels_len), L).sum())
    ctc = nll.sum() / denom
    total = base + weight * ctc
    names = O.trainable_names(P)
    grads = torch.autograd.grad(total, [P[k] for k in names], allow_unused=True)
    grads = {k: (g if g is not None else torch.zeros_like(P[k])).detach().numpy() for k, g in zip(names, grads)}
    gnorm = float(np.sqrt(sum(float(np.sum(g * g)) for g in grads.values())))
    return dict(loss=float(total.detach()), base_loss=float(base.detach()), ctc=float(ctc.detach()), nll=nll.detach().numpy(),
                logits=logits.detach().numpy(), grads=grads, global_norm=gnorm, z=z.detach().numpy())


def best_path(z, in_len, blank):
    """numpy: per-frame argmax (lowest index on ties) over frames t < T_b, repeats collapsed, blanks dropped -> list of id lists."""
    z = np.asarray(z)
    B, T, _C = z.shape
    out = []
    for b in range(B):
        Tb = int(np.clip(in_len[b], 0, T))
        ids = np.argmax(z[b, :Tb], axis=-1) if Tb else np.zeros(0, np.int64)
        seq, prev = [], -1
        for k in ids:
            if k != prev and k != blank:
                seq.append(int(k))
            prev = k
        out.append(seq)
    return out


def brute_force_nll(logp, target, blank):
    """-log of the sum over ALL C^T frame labellings that collapse to `target` (tiny T only); inf when there is none."""
    import itertools
    T, C = logp.shape
    tot = 0.0
    for path in itertools.product(range(C), repeat=T):
        seq, prev = [], -1
        for k in path:
            if k != prev and k != blank:
                seq.append(k)
            prev = k
        if seq == list(target):
            tot += float(np.exp(sum(logp[t, k] for t, k in enumerate(path))))
    return -np.log(tot) if tot > 0 else np.inf
