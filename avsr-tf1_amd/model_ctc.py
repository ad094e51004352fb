"""CTC half of the engine (mixin of model.Seq2SeqModel): the CTC head on the encoder memory, its loss term in the train graph, and the
decodes that need the head alone -- best path, forced alignment, prefix beam search (plain, with a fused avsr.LM network, with a fused
back-off n-gram over the units or over words behind a lexicon trie).  Kernels: csrc/ctc.hip, csrc/ctc_align.hip, csrc/ctc_prefix*.hip; the rules are INTEGRATION.md section 8."""
import numpy as np
import torch
from . import ops
from ._lib import (CTC_ALIGN_MAX_L, CTC_PREFIX_LM_MAX_W, CTC_PREFIX_MAX_L, CTC_PREFIX_MAX_V, CTC_PREFIX_MAX_W, MAX_LM_LAYERS, CtcPrefixLm,
                   CtcPrefixNgram, CtcPrefixWordNgram)


class CtcMixin:
    def _ctc_head(self, ws):
        """z = memory @ kernel + bias over V + 1 classes, on the memory attention sees (_mem_desc)."""
        cfg, B = self.cfg, ws["B"]
        s = cfg.ctc_stream()
        E, Cc = ws["enc"][s], cfg.vocab_size + 1
        ops.gemm(self._mem_desc(ws, s)["vmat"], self.P[f"{s}/ctc/kernel"].mat(Cc), ops.mat(E["ctc_z"], Cc), B * E["T"], Cc,
                 cfg.memory_depth(s), bias=self._pp(f"{s}/ctc/bias"))
        return E, Cc

    def _ctc_forward(self, ws, batch):
        """use_ctc: the head, then avsr_ctc_loss (csrc/ctc.hip): per-utterance ctc_weight * nll / denom added to the step's loss, d logits
        kept for _encode_backward.  The target is the label row without its EOS; the blank is class V."""
        cfg, B = self.cfg, ws["B"]
        E, Cc = self._ctc_head(ws)
        ops.ctc_loss(E["ctc_z"], Cc, batch.labels, batch.labels_len, E["len"], self.denom, cfg.ctc_weight, E["ctc_nll"], E["ctc_status"],
                     E["ctc_utt"], E["ctc_dz"], E["ctc_ws"], B, E["T"], ws["L"], Cc)
        ops.reduce_scalar(E["ctc_utt"], B, self.loss, accumulate=True)

    def ctc_best_path(self, batch):
        """use_ctc: the CTC head's best path -- encoders in evaluation mode, per-frame argmax on the device (frames past an utterance's
        length ignored), repeats collapsed and blanks dropped on the host.  One id list per utterance."""
        return self._redo_if_flagged(self._ctc_best_path, batch)

    def _ctc_best_path(self, batch):
        cfg = self.cfg
        if not cfg.use_ctc:
            raise ValueError("ctc_best_path needs a model built with use_ctc=True")
        ws, B, _Ta, _Tv = self._eval_encode(batch)
        E, Cc = self._ctc_head(ws)
        ops.ctc_best_path(E["ctc_z"], Cc, E["len"], B, E["T"], Cc, E["ctc_ids"])
        ids = E["ctc_ids"].view(B, E["T"]).cpu().numpy()
        out = []
        for row in ids:
            seq, prev = [], -1
            for k in row:
                k = int(k)
                if k < 0:
                    break
                if k != prev and k != Cc - 1:
                    seq.append(k)
                prev = k
            out.append(seq)
        return out

    def ctc_align(self, batch, targets=None):
        """use_ctc: forced alignment on the head (avsr_ctc_align, csrc/ctc_align.hip; the rule is INTEGRATION.md section 8) -- encoders in
        evaluation mode, the head, ONE launch for the batch: the single most probable alignment of a given label sequence to the frames
        of the CTC stream's encoder.  targets=None aligns batch.labels without their EOS; otherwise a list of B id lists (no EOS), for
        example what ctc_prefix_beam_search or attention_rescoring returned.  One dict per utterance: status (1, or 0 where the labels
        have no valid alignment: score 0.0, empty path and segments), score (log-probability of the alignment), path (the class of every
        frame, blank = vocab_size) and segments, one (label_id, start, end, confidence) per label with start / end the first / last frame
        of its run and confidence = exp(mean log-probability of the run's frames)."""
        return self._redo_if_flagged(self._ctc_align, batch, targets)

    def _ctc_align(self, batch, targets):
        cfg = self.cfg
        if cfg.architecture == "lm":
            raise ValueError("ctc_align: architecture='lm' has no encoder, so no CTC head to align on")
        if not cfg.use_ctc:
            raise ValueError("ctc_align needs a model built with use_ctc=True")
        B = self._batch_rows(batch)
        if targets is None:
            L = int(batch.labels.shape[1])
        else:
            targets = [[int(s) for s in g] for g in targets]
            if len(targets) != B:
                raise ValueError("ctc_align: targets must hold one id list per utterance (got %d lists for a batch of %d)" % (len(targets), B))
            L = max([len(g) for g in targets] + [1])
        if L > CTC_ALIGN_MAX_L:
            raise ValueError("ctc_align: avsr_ctc_align covers targets of up to %d labels (got %d)" % (CTC_ALIGN_MAX_L, L))
        V, dev = cfg.vocab_size, self.dev
        if targets is None:
            labels = batch.labels
            tlen = (batch.labels_len.clamp(0, L) - 1).clamp(min=0).to(torch.int32)     # on the device: the row without its EOS
        else:
            lab = np.zeros((B, L), np.int32)
            for b, g in enumerate(targets):
                lab[b, :len(g)] = g
            labels = torch.as_tensor(lab).to(dev)
            tlen = torch.as_tensor(np.array([len(g) for g in targets], np.int32)).to(dev)
        ws = self._eval_encode(batch)[0]
        E, Cc = self._ctc_head(ws)
        T = E["T"]
        key = ("ctc_align", L)
        if key not in E:
            i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
            E[key] = dict(score=torch.zeros(B, device=dev), status=i32(B), path=i32(B, T), frame_lp=torch.zeros(B, T, device=dev),
                          start=i32(B, L), end=i32(B, L),
                          ws=torch.zeros(ops.ctc_align_ws_bytes(B, T, L) // 8, dtype=torch.int64, device=dev))
        O = E[key]
        ops.ctc_align(E["ctc_z"], Cc, labels, tlen, E["len"], B, T, L, V, O["score"], O["status"], O["path"], O["frame_lp"], O["start"],
                      O["end"], O["ws"])
        score, status, path, lp = (O[k].cpu().numpy() for k in ("score", "status", "path", "frame_lp"))
        start, end, tl, lab = O["start"].cpu().numpy(), O["end"].cpu().numpy(), tlen.cpu().numpy(), labels.cpu().numpy()
        lens = np.clip(E["len"].cpu().numpy(), 0, T)
        out = []
        for b in range(B):
            if not status[b]:
                out.append(dict(status=0, score=0.0, path=[], segments=[]))
                continue
            segs = [(int(lab[b, j]), int(start[b, j]), int(end[b, j]),
                     float(np.exp(np.mean(lp[b, start[b, j]:end[b, j] + 1], dtype=np.float64)))) for j in range(int(tl[b]))]
            out.append(dict(status=1, score=float(score[b]), path=[int(k) for k in path[b, :lens[b]]], segments=segs))
        return out

    def ctc_prefix_beam_search(self, batch, beam_width=10, max_steps=None, nbest=False, lm=None, lm_weight=0.3, length_bonus=0.0,
                               ngram=None, *, word_ngram=None):
        """use_ctc: CTC prefix beam search on the head alone (avsr_ctc_prefix_search, csrc/ctc_prefix.hip; the search of all three forms
        is csrc/ctc_prefix_search.h, the rule is INTEGRATION.md section 8) -- encoders in evaluation mode, the head, ONE launch for the batch; no decoder step.  max_steps bounds the label
        sequences (default: max_label_length).  One id list per utterance, the beam's best; nbest=True: per utterance the whole final
        beam as (ids, score) pairs, best first, score = log p_ctc(ids | x) up to what pruning lost.
        lm: a Seq2SeqModel with architecture='lm' (LSTM) over the same vocabulary -- the model's step runs inside the search's frame
        loop (avsr_ctc_prefix_search_lm, csrc/ctc_prefix_lm.hip): an extension by c also gets lm_weight * log p_lm(c | labels) +
        length_bonus, and the final beam is re-sorted by final = p + lm_weight * log p_lm(EOS | labels).  nbest=True then gives
        (ids, final, s_lm) triples, s_lm = log p_lm(labels, EOS).  Without lm the plain kernel runs and nothing new is allocated.
        ngram: instead of lm, the tables of a back-off n-gram (ngram.compile_tables / ngram.load_tables) -- the same rule and the same
        outputs with lam read from the automaton (avsr_ctc_prefix_search_ngram, csrc/ctc_prefix_ngram.hip); the tables are uploaded
        once per model object.  lm and ngram together are refused.
        word_ngram (keyword only): instead of either, the tables of a WORD-level back-off n-gram behind a lexicon trie
        (ngram.compile_word_tables / ngram.load_word_tables) for a model over single-character units -- the same rule and outputs with
        lam formed from the trie while a word is written and from the word automaton when a space or EOS closes it
        (avsr_ctc_prefix_search_word_ngram, csrc/ctc_prefix_word_ngram.hip); uploaded once per model object.  Refused together with
        lm or ngram."""
        kw = {} if word_ngram is None else dict(word_ngram=word_ngram)
        return self._redo_if_flagged(self._ctc_prefix_beam_search, batch, beam_width, max_steps, nbest, lm, lm_weight, length_bonus, ngram,
                                     **kw)

    def _ctc_prefix_beam_search(self, batch, beam_width, max_steps, nbest, lm=None, lm_weight=0.3, length_bonus=0.0, ngram=None,
                                word_ngram=None):
        cfg = self.cfg
        if not cfg.use_ctc:
            raise ValueError("ctc_prefix_beam_search needs a model built with use_ctc=True")
        W, V = int(beam_width), cfg.vocab_size
        Lm = int(cfg.max_label_length if max_steps is None else max_steps)
        self._require_ctc_prefix_shape("ctc_prefix_beam_search", V, W, Lm)
        if lm is not None and ngram is not None:
            raise ValueError("ctc_prefix_beam_search takes one language model: lm (an avsr.LM network) or ngram (back-off tables), not both")
        if word_ngram is not None and (lm is not None or ngram is not None):
            raise ValueError("ctc_prefix_beam_search takes one language model: word_ngram (word-level tables behind a lexicon) cannot "
                             "be combined with lm or ngram")
        if lm is not None:
            self._check_lm(lm)
        if lm is not None or ngram is not None or word_ngram is not None:
            lm_weight, length_bonus = self._require_weight("ctc_prefix_beam_search", "lm_weight", float(lm_weight)), float(length_bonus)
            if length_bonus != length_bonus or abs(length_bonus) == float("inf"):
                raise ValueError("ctc_prefix_beam_search: length_bonus must be finite (got %r)" % (length_bonus,))
        if ngram is not None:
            if (ngram["V"], ngram["go_id"], ngram["eos_id"]) != (V, cfg.go_id, cfg.eos_id):
                raise ValueError("ctc_prefix_beam_search: the n-gram tables were compiled for V = %d, GO = %d, EOS = %d; the model has %d, "
                                 "%d, %d" % (ngram["V"], ngram["go_id"], ngram["eos_id"], V, cfg.go_id, cfg.eos_id))
            if not ops.ctc_prefix_ngram_supported(V, W, Lm, ngram["n_nodes"], ngram["n_arcs"]):
                raise ValueError("ctc_prefix_beam_search: with an n-gram avsr_ctc_prefix_search_ngram covers beam widths of up to %d "
                                 "(vocabularies of up to %d symbols, label sequences of up to %d) and automata of up to %d nodes and %d "
                                 "arcs (got beam width %d, %d symbols, %d labels, %d nodes, %d arcs)"
                                 % (CTC_PREFIX_LM_MAX_W, CTC_PREFIX_MAX_V, CTC_PREFIX_MAX_L, 1 << 24, 1 << 26, W, V, Lm,
                                    ngram["n_nodes"], ngram["n_arcs"]))
        if word_ngram is not None:
            g = word_ngram
            if (g["V"], g["go_id"], g["eos_id"]) != (V, cfg.go_id, cfg.eos_id):
                raise ValueError("ctc_prefix_beam_search: the word n-gram tables were compiled for V = %d, GO = %d, EOS = %d; the model has "
                                 "%d, %d, %d" % (g["V"], g["go_id"], g["eos_id"], V, cfg.go_id, cfg.eos_id))
            if not ops.ctc_prefix_word_ngram_supported(V, W, Lm, g["n_nodes"], g["n_arcs"], g["Vw"], g["n_trie_nodes"], g["n_trie_arcs"]):
                raise ValueError("ctc_prefix_beam_search: with a word n-gram avsr_ctc_prefix_search_word_ngram covers beam widths of up to "
                                 "%d (vocabularies of up to %d symbols, label sequences of up to %d) and word automata and lexicon tries "
                                 "of up to %d nodes and %d arcs each (got beam width %d, %d symbols, %d labels, %d nodes, %d arcs, %d "
                                 "trie nodes, %d trie arcs)"
                                 % (CTC_PREFIX_LM_MAX_W, CTC_PREFIX_MAX_V, CTC_PREFIX_MAX_L, 1 << 24, 1 << 26, W, V, Lm, g["n_nodes"],
                                    g["n_arcs"], g["n_trie_nodes"], g["n_trie_arcs"]))
        if lm is not None:
            lc = lm.cfg
            nl, H, El = len(lc.decoder_units), lc.decoder_units[0], lc.embedding_size
            if not ops.ctc_prefix_lm_supported(V, W, Lm, nl, H, El, int(lm.onehot is not None)):
                raise ValueError("ctc_prefix_beam_search: with a language model avsr_ctc_prefix_search_lm covers beam widths of up to %d "
                                 "(vocabularies of up to %d symbols, label sequences of up to %d) and LSTM models of up to %d equal layers "
                                 "(got beam width %d, %d symbols, %d labels, %d layers of %d units)"
                                 % (CTC_PREFIX_LM_MAX_W, CTC_PREFIX_MAX_V, CTC_PREFIX_MAX_L, MAX_LM_LAYERS, W, V, Lm, nl, H))
        ws, B, _Ta, _Tv = self._eval_encode(batch)
        E, Cc = self._ctc_head(ws)
        ids, lens, score = self._ctc_nbest_buffers(E, B, W, Lm)
        s_lm = None                                                # (device) with a model: the third column of the n-best
        if word_ngram is not None:
            s_lm = self._ctc_prefix_word_ngram_launch(E, Cc, B, V, W, Lm, ids, lens, score, word_ngram, lm_weight, length_bonus)
        elif ngram is not None:
            s_lm = self._ctc_prefix_ngram_launch(E, Cc, B, V, W, Lm, ids, lens, score, ngram, lm_weight, length_bonus)
        elif lm is not None:
            s_lm = self._ctc_prefix_lm_launch(E, Cc, B, V, W, Lm, ids, lens, score, lm, lm_weight, length_bonus)
        else:
            ops.ctc_prefix_search(E["ctc_z"], Cc, E["len"], B, E["T"], V, W, Lm, ids, lens, score)
        cols = [score.cpu().numpy()] + ([] if s_lm is None else [s_lm.cpu().numpy()])
        ids, lens = ids.cpu().numpy(), lens.cpu().numpy()
        if not nbest:
            return [[int(s) for s in ids[b, 0, :lens[b, 0]]] for b in range(B)]
        return [[([int(s) for s in ids[b, r, :lens[b, r]]],) + tuple(float(c[b, r]) for c in cols) for r in range(W)
                 if cols[0][b, r] > float("-inf")] for b in range(B)]

    @staticmethod
    def _require_ctc_prefix_shape(who, V, W, Lm):
        """What avsr_ctc_prefix_search covers, refused in the name of the decode `who` (the search itself, attention rescoring)."""
        if W < 1 or Lm < 1:
            raise ValueError("%s: beam_width and max_steps must be positive (got %d, %d)" % (who, W, Lm))
        if not ops.ctc_prefix_search_supported(V, W, Lm):
            raise ValueError("%s: avsr_ctc_prefix_search covers vocabularies of up to %d symbols, beam widths of up to "
                             "%d and label sequences of up to %d (got %d, %d, %d)"
                             % (who, CTC_PREFIX_MAX_V, CTC_PREFIX_MAX_W, CTC_PREFIX_MAX_L, V, W, Lm))

    def _ctc_nbest_buffers(self, E, B, W, Lm):
        """E[("ctc_prefix", W, Lm)], the cached n-best of a prefix search on this workspace: ids [B, W, Lm], lens [B, W], score [B, W]
        (device), made on first use; the fused searches keep their own outputs next to it (_ctc_prefix_model_outputs)."""
        key = ("ctc_prefix", W, Lm)
        if key not in E:
            dev = self.dev
            E[key] = (torch.zeros(B, W, Lm, dtype=torch.int32, device=dev), torch.zeros(B, W, dtype=torch.int32, device=dev),
                      torch.zeros(B, W, device=dev))
        return E[key]

    def _ctc_prefix_model_outputs(self, E, key, B, W):
        """E[key], the cached buffers of a fused search: s_lm [B, W] and steps [B], made on first use."""
        if key not in E:
            E[key] = dict(s_lm=torch.zeros(B, W, device=self.dev), steps=torch.zeros(B, dtype=torch.int32, device=self.dev))
        return E[key]

    def _ctc_prefix_lm_launch(self, E, Cc, B, V, W, Lm, ids, lens, score, lm, lm_weight, length_bonus):
        """avsr_ctc_prefix_search_lm over the language model's own (4-padded) weights; the state workspace, s_lm and lm_steps are
        cached next to the ("ctc_prefix", W, Lm) buffers, keyed by the model's shape.  Returns s_lm [B, W] (device)."""
        lc, m = lm.cfg, CtcPrefixLm()
        self._fill_lm_weights(m, lm)
        nl, H = m.n_layers, m.H                                    # (m.V is the model's own: _check_lm has it equal to V)
        buf = self._ctc_prefix_model_outputs(E, ("ctc_prefix_lm", W, Lm, nl, H), B, W)
        if "ws" not in buf:
            buf["ws"] = torch.zeros(ops.ctc_prefix_lm_ws_bytes(B, W, nl, H) // 4, device=self.dev)
        m.go_id, m.eos_id, m.weight, m.bonus = lc.go_id, lc.eos_id, lm_weight, length_bonus
        m.ws, m.ws_bytes = ops.fptr(buf["ws"]), buf["ws"].numel() * 4
        m.s_lm, m.lm_steps = ops.fptr(buf["s_lm"]), ops.fptr(buf["steps"])
        ops.ctc_prefix_search_lm(E["ctc_z"], Cc, E["len"], B, E["T"], V, W, Lm, ids, lens, score, m)
        self._last_ctc_lm_steps = buf["steps"]
        return buf["s_lm"]

    def _ctc_prefix_ngram_launch(self, E, Cc, B, V, W, Lm, ids, lens, score, ngram, lm_weight, length_bonus):
        """avsr_ctc_prefix_search_ngram over the automaton `ngram` (ngram.compile_tables): its six arrays go to the device once per
        model object (kept with the dict they came from); s_lm and lm_steps are cached next to the ("ctc_prefix", W, Lm) buffers.
        Returns s_lm [B, W] (device)."""
        tb = self._ngram_device_tables(ngram)
        buf = self._ctc_prefix_model_outputs(E, ("ctc_prefix_ngram", W, Lm), B, W)
        g = CtcPrefixNgram()
        g.n_nodes, g.n_arcs, g.V, g.start = int(ngram["n_nodes"]), int(ngram["n_arcs"]), V, int(ngram["start"])
        g.go_id, g.eos_id, g.weight, g.bonus = int(ngram["go_id"]), int(ngram["eos_id"]), lm_weight, length_bonus
        for k in self.NGRAM_TABLES:
            setattr(g, k, ops.fptr(tb[k]))
        g.s_lm, g.lm_steps = ops.fptr(buf["s_lm"]), ops.fptr(buf["steps"])
        ops.ctc_prefix_search_ngram(E["ctc_z"], Cc, E["len"], B, E["T"], V, W, Lm, ids, lens, score, g)
        self._last_ctc_lm_steps = buf["steps"]
        return buf["s_lm"]

    WORD_NGRAM_TABLES = ("bow", "backoff", "arc_begin", "sym", "logp", "next", "t_begin", "t_sym", "t_next", "t_word")

    def _ctc_prefix_word_ngram_launch(self, E, Cc, B, V, W, Lm, ids, lens, score, tables, lm_weight, length_bonus):
        """avsr_ctc_prefix_search_word_ngram over the word automaton and lexicon trie `tables` (ngram.compile_word_tables): the ten
        arrays go to the device once per model object (_ngram_device_tables); s_lm and lm_steps are cached next to the
        ("ctc_prefix", W, Lm) buffers.  Returns s_lm [B, W] (device)."""
        tb = self._ngram_device_tables(tables, self.WORD_NGRAM_TABLES)
        buf = self._ctc_prefix_model_outputs(E, ("ctc_prefix_word_ngram", W, Lm), B, W)
        g = CtcPrefixWordNgram()
        for k in ("n_nodes", "n_arcs", "Vw", "start", "eos_w", "unk_id", "n_trie_nodes", "n_trie_arcs", "space_id", "go_id", "eos_id"):
            setattr(g, k, int(tables[k]))
        g.V, g.weight, g.bonus, g.oov = V, lm_weight, length_bonus, float(tables["oov_score"])
        for k in self.WORD_NGRAM_TABLES:
            setattr(g, k, ops.fptr(tb[k]))
        g.s_lm, g.lm_steps = ops.fptr(buf["s_lm"]), ops.fptr(buf["steps"])
        ops.ctc_prefix_search_word_ngram(E["ctc_z"], Cc, E["len"], B, E["T"], V, W, Lm, ids, lens, score, g)
        self._last_ctc_lm_steps = buf["steps"]
        return buf["s_lm"]
