"""Containers and small helpers shared by the engine's modules (model.py, model_encoder.py, model_decoder.py, model_ctc.py,
model_rescore.py): the device batch, views into the flat parameter buffers, sequence buffers with guard slots, the flag reader of the
decode loops, and EvalMixin: the one copy of every step the evaluation decodes share."""
from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, List, Optional
import os
import numpy as np
import torch
from . import ops, params as PR
from ._lib import AttnRnn, RnnStack
from .config import ATT_CODE, BAHDANAU_TYPES, CELL_ID_DECODER, LUONG_TYPES, ModelConfig, encoder_cell_id


@dataclass
class Batch:
    """Device-side BatchedData (avsr/io_utils.py:8-18).  float32 [B,T,F] inputs, int32 lengths/labels."""
    audio: Optional[torch.Tensor] = None
    audio_len: Optional[torch.Tensor] = None
    video: Optional[torch.Tensor] = None
    video_len: Optional[torch.Tensor] = None
    aus: Optional[torch.Tensor] = None
    labels: Optional[torch.Tensor] = None
    labels_len: Optional[torch.Tensor] = None

    @staticmethod
    def from_numpy(b, device="cuda"):
        def f(a, dt):
            return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(device).contiguous()
        return Batch(f(getattr(b, "audio", None), torch.float32), f(getattr(b, "audio_len", None), torch.int32),
                     f(getattr(b, "video", None), torch.float32), f(getattr(b, "video_len", None), torch.int32),
                     f(getattr(b, "aus", None), torch.float32), f(getattr(b, "labels", None), torch.int32),
                     f(getattr(b, "labels_len", None), torch.int32))


class Ref:
    """A named slice of a flat device buffer."""

    def __init__(self, t, off, shape):
        self.t, self.off, self.shape = t, int(off), tuple(shape)
        self.n = int(np.prod(shape))

    def mat(self, ld=None, row0=0, col0=0):
        ld = self.shape[-1] if ld is None else ld
        return ops.mat(self.t, ld, offset=self.off + row0 * ld + col0)

    def view(self):
        return self.t[self.off:self.off + self.n].view(*self.shape)


class SeqBuf:
    """[B, lead + T + trail, D] sequence buffer; time t lives in slot lead + t; guard slots stay zero."""

    def __init__(self, B, T, D, lead, trail, device):
        self.B, self.T, self.D, self.lead = B, T, D, lead
        self.slots = lead + T + trail
        self.t = torch.zeros(B, self.slots, D, device=device)
        self.sb, self.st = self.slots * D, D

    def off(self, dt=0, col=0):
        return (self.lead + dt) * self.D + col

    def mat(self, dt=0, col=0):
        return ops.mat(self.t, self.D, T=self.T, ldo=self.sb, offset=self.off(dt, col))


def _splitk(M, N, K):
    return ops.auto_splitk(M, N, K)


class _FlagReader:
    """Reads a device int32 word for the host WITHOUT draining the main stream: the word is copied to page-locked memory on a side
    stream behind an event, so a decode loop can queue its next chunk of steps before it looks at the previous chunk's "all finished"
    counter (a plain .item() waits for everything queued so far, the next chunk included)."""

    def __init__(self, device):
        self.side = torch.cuda.Stream(device=device)
        self.host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self.done = torch.cuda.Event()

    def request(self, word):
        """Queue the read of `word` (a 1-element int32 device tensor) as of everything queued on the current stream so far."""
        ev = torch.cuda.Event()
        ev.record()
        with torch.cuda.stream(self.side):
            self.side.wait_event(ev)
            self.host.copy_(word, non_blocking=True)
            self.done.record()

    def value(self):
        self.done.synchronize()
        return int(self.host[0])


def desc_steplen(desc):
    return _PtrView(desc.steplen)


class _PtrView:
    """Wraps a raw device address so it can be passed where ops.fptr() expects a tensor."""

    def __init__(self, addr):
        self.addr = addr
        self.is_cuda = True

    def data_ptr(self):
        return self.addr

    def element_size(self):
        return 4


class EvalMixin:
    """Steps shared by the evaluation decodes (mixin of model.Seq2SeqModel): greedy, beam search, the CTC decodes, attention rescoring."""

    @staticmethod
    def _batch_rows(batch):
        return next(x for x in (batch.audio, batch.video, batch.labels) if x is not None).shape[0]

    def _eval_encode(self, batch, L=1):
        """Prologue of an evaluation decode: the workspace of the batch's shape (decoder block of L steps; the searches that bring
        their own block pass 1), the transposed operands, the encoders in evaluation mode.  Returns (ws, B, Ta, Tv)."""
        B = self._batch_rows(batch)
        Ta = self._audio_rows(batch)
        Tv = batch.video.shape[1] if batch.video is not None else 0
        ws = self._get_ws(B, Ta, Tv, L, True)
        self._refresh_derived()
        self._encode(ws, batch, False)
        return ws, B, Ta, Tv

    def _redo_if_flagged(self, fn, *args, **kw):
        """fn(*args, **kw); if a persistent kernel's bounded wait expired during the pass (workgroups not co-resident) its results are
        invalid: check_persistent() has then switched the one-launch paths off, and the pass is redone through the per-step launches."""
        out = fn(*args, **kw)
        if self.check_persistent():
            out = fn(*args, **kw)
        return out

    def persistent_flagged(self):
        """Read-only form of check_persistent(): did a persistent kernel flag the last pass on THIS rank?"""
        return bool(self.persistent_rnn and ops.rnn_persistent_error())

    def check_persistent(self, disable=True, force=False):
        """Synchronise and read the persistent kernels' sticky error word (a bounded device-side wait expired: some
        workgroups were not co-resident).  Returns True if the last results are invalid; the persistent path is then
        switched off so that the caller can simply redo the pass through the per-step launches.  force=True: another
        data-parallel rank flagged its pass -- switch off here as well so that every rank redoes the pass the same way."""
        if not self.persistent_rnn:
            return False
        if not force and not ops.rnn_persistent_error():
            return False
        if disable:
            import warnings
            warnings.warn("avsr_tf1_amd: persistent RNN kernel timed out; falling back to per-step launches")
            self.persistent_rnn = False
            self.fused_decode = False
            ops.rnn_set_persistent(False)
            ops.rnn_persistent_clear()
        return True

    def _sp(self, name):
        """The non-trainable buffer `name` (batch-norm moving statistics) as the kernels update it.  While a flagged pass is being REDONE
        (redoing()) the updates go to a scratch copy: every batch norm sits upstream of the persistent kernels, so the flagged pass
        has already applied this step's (valid) update, and a second one would move the averages twice in one step."""
        r = self.S[name]
        if self._redo_pass:
            if self._stats_sink is None:
                self._stats_sink = torch.empty_like(self.stats)
            ops.copy_(self._stats_sink[r.off:r.off + r.n], r.t[r.off:r.off + r.n])      # (the kernels read the old value to blend it)
            return self._stats_sink[r.off:r.off + r.n]
        return r.t[r.off:r.off + r.n]

    def redoing(self):
        """Context of a pass that repeats one whose persistent kernels flagged (trainer / decode redo paths): see _sp."""
        import contextlib

        @contextlib.contextmanager
        def ctx():
            self._redo_pass = True
            try:
                yield
            finally:
                self._redo_pass = False
        return ctx()

    @staticmethod
    def _require_weight(who, name, value):
        """float(value), refused unless it is a finite number >= 0 (the message shows `value` as it was given)."""
        w = float(value)
        if not w >= 0.0 or w == float("inf"):
            raise ValueError("%s: %s must be a finite number >= 0 (got %r)" % (who, name, value))
        return w

    NGRAM_TABLES = ("bow", "backoff", "arc_begin", "sym", "logp", "next")

    def _ngram_device_tables(self, ngram, names=NGRAM_TABLES):
        """The six arrays of the automaton `ngram` (ngram.compile_tables) on the device: uploaded once per model object and kept with the
        dict they came from, for every search that fuses it (the CTC prefix search, beam search)."""
        cache = self.__dict__.setdefault("_ngram_tables", {})
        if id(ngram) not in cache:
            cache[id(ngram)] = (ngram, {k: torch.as_tensor(np.ascontiguousarray(ngram[k])).to(self.dev) for k in names})
        return cache[id(ngram)][1]

    @staticmethod
    def _fill_lm_weights(m, lm):
        """The language model's own (4-padded) weights into a BeamLm or a CtcPrefixLm: the two descriptors share these field names."""
        lc = lm.cfg
        lm._refresh_derived()
        m.n_layers, m.H, m.E, m.V, m.one_hot = len(lc.decoder_units), lc.decoder_units[0], lc.embedding_size, lc.vocab_size, int(lm.onehot is not None)
        m.embedding = ops.fptr(*lm._emb())
        for j in range(m.n_layers):
            m.wt[j] = ops.fptr(lm.derived, lm.Tr["dec/l%d/kernel" % j].off)
            m.bias[j] = ops.fptr(lm.params, lm.P["dec/l%d/bias" % j].off)
        m.wout_t = ops.fptr(lm.derived, lm.Tr["dec/out/kernel"].off)
        m.bout = ops.fptr(lm.params, lm.P["dec/out/bias"].off)
