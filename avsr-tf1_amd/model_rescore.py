"""Attention rescoring of the CTC n-best (mixin of model.Seq2SeqModel): the two-pass decode of a hybrid CTC / attention model.  The CTC
head's prefix beam search (csrc/ctc_prefix.hip, model_ctc.py) proposes, the attention decoder scores every proposal teacher-forced (the train graph's
decoder block, mode 0, evaluation settings), avsr_seq_logprob / avsr_rescore_select (csrc/rescore.hip) score and choose.  The rule is this
project's own: INTEGRATION.md section 8.  No reference counterpart."""
import numpy as np
import torch
from . import ops

RESCORE_MAX_BLOCKS = 4        # decoder blocks (one per padded hypothesis length and width) an encoder workspace keeps


class RescoreMixin:
    def attention_rescoring(self, batch, beam_width=10, max_steps=None, ctc_weight=0.0, nbest=False):
        """use_ctc: per utterance the hypothesis of the CTC prefix search's final beam (width beam_width, L_max = max_steps, default
        max_label_length -- exactly ctc_prefix_beam_search(nbest=True)) with the largest
            final = s_att + ctc_weight * s_ctc,
        s_att = sum_t log_softmax(logits[t])[label[t]] of the attention decoder run teacher-forced on `ids . EOS`, s_ctc the search's
        score; ties go to the better CTC rank; no length normalisation, no language-model term; ctc_weight = 0 forms no product.
        Returns one id list per utterance; nbest=True: per utterance every hypothesis as (ids, final, s_att, s_ctc), sorted by final
        descending (ties: CTC rank).
        Encoders (evaluation mode: moving statistics untouched) and the head run once; the decoder passes -- one per n-best rank, row b of
        pass k = hypothesis k of utterance b, labels_len 0 where the utterance has fewer -- share the workspace's memories, their keys and
        the initial state.  Teacher forcing (mode 0) and keep-probabilities of 1 whatever sampling_probability / use_dropout the model
        was built with; the step counter, the dropout seed, the loss, the gradient buffers and forward_train's own state are not touched.
        The label rows are padded to Lh = the batch's longest hypothesis + 1 ROUNDED UP TO A MULTIPLE OF 8, which bounds the number of
        decoder blocks a workspace ever sees (the RESCORE_MAX_BLOCKS most recent are kept).
        A pass a persistent kernel flagged is redone through the per-step launches, as for the other decodes."""
        return self._redo_if_flagged(self._attention_rescoring, batch, beam_width, max_steps, ctc_weight, nbest)

    def _attention_rescoring(self, batch, beam_width, max_steps, ctc_weight, nbest):
        cfg, dev = self.cfg, self.dev
        if cfg.architecture == "lm":
            raise ValueError("attention_rescoring: architecture='lm' has no encoder, so no CTC head whose n-best could be rescored")
        if not cfg.use_ctc:
            raise ValueError("attention_rescoring needs a model built with use_ctc=True: the hypotheses are the CTC head's n-best")
        w = self._require_weight("attention_rescoring", "ctc_weight", ctc_weight)
        K, V = int(beam_width), cfg.vocab_size
        Lm = int(cfg.max_label_length if max_steps is None else max_steps)
        self._require_ctc_prefix_shape("attention_rescoring", V, K, Lm)
        ws, B, Ta, Tv = self._eval_encode(batch)               # encoders at batch B (the decoder block of this workspace is unused)
        # ---- first pass: the head's n-best, as ctc_prefix_beam_search(nbest=True) (same buffers) ---------------------------------
        E, Cc = self._ctc_head(ws)
        ids_d, lens_d, s_ctc_d = self._ctc_nbest_buffers(E, B, K, Lm)
        ops.ctc_prefix_search(E["ctc_z"], Cc, E["len"], B, E["T"], V, K, Lm, ids_d, lens_d, s_ctc_d)
        ids, lens, s_ctc = ids_d.cpu().numpy(), lens_d.cpu().numpy(), s_ctc_d.cpu().numpy()
        real = s_ctc > float("-inf")                           # empty slots are not hypotheses
        n = real.sum(1).astype(np.int32)
        assert (n >= 1).all() and all(real[b, :n[b]].all() for b in range(B)), "the prefix search's beam is sorted: real entries first"
        kmax = int(n.max())
        # ---- label rows ids . EOS, [K][B][Lh], uploaded once ----------------------------------------------------------------------
        Lh = (int((lens * real).max()) + 1 + 7) // 8 * 8
        labels = np.zeros((K, B, Lh), np.int32)
        llen = np.zeros((K, B), np.int32)
        for b in range(B):
            for k in range(int(n[b])):
                l = int(lens[b, k])
                labels[k, b, :l] = ids[b, k, :l]
                labels[k, b, l] = cfg.eos_id
                llen[k, b] = l + 1
        labels_d, llen_d, n_d = (torch.from_numpy(a).to(dev) for a in (labels, llen, n))
        # ---- second pass: the train graph's decoder, teacher-forced, once per rank -------------------------------------------------
        D = self._rescore_block(ws, B, Lh, K, Ta, Tv)
        wsr = {"enc": ws["enc"], "dec": D, "B": B, "L": Lh}
        D["s_att"].zero_()
        for k in range(kmax):
            lg = self._decoder_train_pass(wsr, D, labels_d[k], llen_d[k], False, with_bwd=False, prepare=(k == 0), logits=D["logits_k"][k])
            ops.seq_logprob(lg, labels_d[k], llen_d[k], B, Lh, V, D["s_att"], out_stride=K, out_offset=k)
        ops.rescore_select(D["s_att"], s_ctc_d, n_d, B, K, w, D["order"], D["final"])
        order, final, s_att = D["order"].cpu().numpy(), D["final"].cpu().numpy(), D["s_att"].cpu().numpy()
        self._last_rescore = dict(ws=wsr, labels=labels, labels_len=llen, n=n, Lh=Lh, K=K)       # (tests read the logits back)
        out = []
        for b in range(B):
            rows = []
            for r in range(int(n[b])):
                k = int(order[b, r])
                rows.append(([int(s) for s in ids[b, k, :lens[b, k]]], float(final[b, r]), float(s_att[b, k]), float(s_ctc[b, k])))
            out.append(rows)
        return out if nbest else [rows[0][0] for rows in out]

    def _rescore_block(self, ws, B, Lh, K, Ta, Tv):
        """The decoder block of the teacher-forced passes (one memory per row, as the train graph's) with the buffers around it, kept
        in the encoder workspace it attends.  _make_block also allocates the block's backward records, which no pass here reads (at the
        c2 shape some 0.4 GB per block); the RESCORE_MAX_BLOCKS cap bounds what a workspace holds."""
        cfg, dev = self.cfg, self.dev
        cache = ws.setdefault("rescore", {})
        key = (Lh, K)
        if key in cache:
            cache[key] = cache.pop(key)                        # most recently used last
            return cache[key]
        while len(cache) >= RESCORE_MAX_BLOCKS:
            cache.pop(next(iter(cache)))
        mems, V = cfg.decoder_memories(), cfg.vocab_size
        D = self._make_block(ws, B, Lh, cfg.decoder_units[0], cfg.embedding_size, mems, "dec/l0",
                             ["dec/att%d" % i for i in range(len(mems))], Tv=Tv, Ta=Ta, greedy=True)
        D["xemb"] = torch.zeros(B * Lh, cfg.embedding_size, device=dev)
        D["fed"] = torch.zeros(B, Lh, dtype=torch.int32, device=dev)
        D["logits_k"] = torch.zeros(K, B, Lh, V, device=dev)
        D["s_att"], D["final"] = torch.zeros(B, K, device=dev), torch.zeros(B, K, device=dev)
        D["order"] = torch.zeros(B, K, dtype=torch.int32, device=dev)
        cache[key] = D
        return D
