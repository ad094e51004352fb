"""`AVSR` -- the reference's top-level class (avsr/avsr.py:20-753) on the MI355X engine.

Same constructor keywords and defaults (avsr/avsr.py:21-75), same `train(logfile, num_epochs,
try_restore_latest_checkpoint)` / `evaluate(checkpoint_path, epoch)` behaviour and side-effect files:
`logs/<logfile>` (average loss per epoch, error rates every 10th epoch), `checkpoints/<name>/checkpoint.ckp-<epoch>`
(own .npz format: TF-layout weights + Adam slots + step; epoch parsed from the file name on resume, :233-249),
`predictions/<name>/predicted_epoch_<N>.mlf`.  TensorFlow graphs/sessions/summaries do not exist here.

`video_processing='resnet_cnn'` runs the lip crops through the HIP lip-CNN front-end (cnn.py; avsr/video.py:143-195);
`video_processing='3dconv_cnn'` through the spatio-temporal front-end (cnn3d.py, csrc/conv3d.hip; avsr/video.py:198-222), whose final
conv3d is built with strides (1, 1, 1) where the reference passes (1, 1).
Built besides the defaults: `input_dense_layers`, `instance_normalisation`, `residual_encoder`, `highway_encoder`, `encoder_weight_sharing`, multi-layer
decoders (equal widths), `enable_attention=False`, `loss_fun` / `label_smoothing`, `lr_decay=('cosine_restarts', N)`, the Nadam /
AdamW / Momentum optimisers, `write_attention_alignment` (greedy decoding), one-hot decoder inputs (`embedding_size <= 0`).  Feature / unit /
embedding sizes may be anything (the engine pads to multiples of 4 inside, config.py `engine()`; checkpoints keep the reference's shapes).
`audio_processing='wav'` takes waveform records (one float per step) and runs the dataset writer's log-mel pipeline inside the model
(audio_frontend.py, csrc/audio_frontend.hip); keywords `audio_transformation` ('logmel_stack_w8s3' | 'logmel_stack_w3s3' | 'logmel'),
`num_mel_bins` (30) and `sample_rate` (16000) arrive through **kwargs.  The reference's own 'wav' branch (avsr/avsr.py:719-724) omits
`need_logmel`, so its encoder would get the complex STFT with lengths in samples and cannot train; the engine computes what the writer
computes instead.
Not built (raise explicitly): `precision='float16'`, the `2dconv_cnn` front-end, `sync_cnn_bn` data parallelism with `3dconv_cnn`, the
writer's MFCC / delta audio transformations, the monotonic attention variants and the non-default cell types.
Shallow fusion of a language model into beam search (not in the reference, which trains `avsr.LM` but never uses it in the recogniser):
`lm_checkpoint` (a checkpoint written by `LM.train`), `lm_weight` (0.3: a conventional value, not a tuned one),
`lm_units_per_layer` ((256,)), `lm_embedding_size` (128), `lm_cell_type` ('lstm') arrive through **kwargs; `evaluate` then scores an
unfinished beam's continuation with log p_model + lm_weight * log p_lm (csrc/beam_lm.hip).
`ngram_lm` (the path of an ARPA file over the units, read as `ctc_ngram_lm` below is) fuses a back-off n-gram into beam search instead,
with the same `lm_weight`: log p_model + lm_weight * lam(v | GO, labels), one table-walk launch per step and no model to train
(ngram.py, csrc/beam_ngram.hip).  It is refused together with `lm_checkpoint` and under any other `decoding_algorithm`; it works together
with `ctc_decode_weight`.
`word_ngram_lm` (the path of an ARPA file over WORDS, read as `ctc_word_ngram_lm` below is) fuses a word-level back-off n-gram into beam
search of a model over single-character units through a lexicon trie, again with `lm_weight`: letters inside the lexicon are free, the
letter that leaves it pays `word_oov_score` (-10.0, natural log: a conventional value, not a tuned one) once, and a space or EOS that
closes a word pays the word model (ngram.py compile_word_tables, csrc/beam_word_ngram.hip; the rule is INTEGRATION.md section 8).  No CTC
head is needed.  Refused together with `lm_checkpoint` or `ngram_lm`, under any other `decoding_algorithm`, and for unit files without
' ' or with multi-character units; it works together with `ctc_decode_weight`.  Nothing was trained with it: no error rate is claimed.
Hybrid CTC / attention training (not in the reference, which only reserves `use_ctc` in its hyper-parameters): `use_ctc` (False),
`ctc_weight` (0.3: a conventional value, not a tuned one) arrive through **kwargs; a CTC head on the audio (else video) encoder adds
ctc_weight * CTC loss per label token to the step's loss, and `evaluate` also reports that head's best-path error rate under the key
'ctc_' + unit (csrc/ctc.hip).  `ctc_decode_weight` (0.0 = off) is an evaluate-time option of a `use_ctc` model:
beam search then adds ctc_decode_weight * (CTC prefix score of the continuation - that of the beam) to an unfinished beam's step score
(joint CTC / attention decoding, csrc/beam_ctc.hip); it works together with `lm_checkpoint`.
`decoding_algorithm='ctc_prefix_beam_search'` (a `use_ctc` model; not in the reference) makes `evaluate` take its predictions from a CTC
prefix beam search of width `beam_width` on that head alone -- no decoder step (csrc/ctc_prefix.hip; the search itself,
shared with the two fused forms below, is csrc/ctc_prefix_search.h).
`ctc_lm_checkpoint` (a checkpoint written by `LM.train`; the model's shape through `lm_units_per_layer` / `lm_embedding_size` /
`lm_cell_type`), `ctc_lm_weight` (0.3: a conventional value, not a tuned one) and `ctc_lm_length_bonus` (0.0) arrive through **kwargs and
fuse that language model INTO this search: an extension by c also gets ctc_lm_weight * log p_lm(c | labels) + ctc_lm_length_bonus, and the
final beam is re-sorted with ctc_lm_weight * log p_lm(EOS | labels) added (csrc/ctc_prefix_lm.hip; beam widths
of up to 16).  `lm_checkpoint` itself stays a 'beam_search' option.
`ctc_ngram_lm` (the path of an ARPA file over the units: <s> = GO, </s> = EOS, <space> = ' ', every other token a unit's string) fuses a
back-off n-gram into the same search instead, with the same two weights (ngram.py, csrc/ctc_prefix_ngram.hip): a table walk per kept
extension, no weight-matrix product.  It is refused together with `ctc_lm_checkpoint` and under any other `decoding_algorithm`.
`ctc_word_ngram_lm` (the path of an ARPA file over WORDS: <s>, </s>, optionally <unk>, every other token a word spelled by its own
characters) fuses a word-level back-off n-gram into the same search of a model over single-character units, again with the same two
weights: a trie over the spellings follows the word being written, and the word model is consulted when a space or the end closes it
(ngram.py compile_word_tables, csrc/ctc_prefix_word_ngram.hip; the rule is INTEGRATION.md section 8).  `ctc_word_oov_score` (-10.0,
natural log: a conventional value, not a tuned one) is paid once by a word that leaves the lexicon.  Refused together with
`ctc_lm_checkpoint` or `ctc_ngram_lm`, under any other `decoding_algorithm`, with `beam_width` > 16, and for unit files without ' ' or
with multi-character units.  Nothing was trained with it: no error rate is claimed.
`decoding_algorithm='attention_rescoring'` (a `use_ctc` model; not in the reference) is the two-pass decode: that search's n-best, every
hypothesis scored by the attention decoder teacher-forced, the best of log p_att + ctc_decode_weight * log p_ctc kept -- no step-by-step
decode (csrc/rescore.hip).  No language-model term, no length normalisation.
`AVSR.align` (a `use_ctc` model; not in the reference) returns and writes the forced alignment of every evaluate utterance's labels, or of
its predictions, on the CTC head: per label the first and last frame and a confidence (csrc/ctc_align.hip).
`spec_augment` (None = off, or a dict; not in the reference, which only mixes noise offline in its dataset writer) arrives through
**kwargs and masks the encoders' inputs inside the train step, anew every step: `freq_masks` bands of up to `freq_width` of the
`freq_bins` bins and `time_masks` spans of up to min(`time_width`, `time_ratio` * length) rows on the audio stream,
`video_time_masks` / `video_time_width` / `video_time_ratio` spans of frames on the video stream (features or lip crops), filled with
`mask_value` = 'mean' (the utterance's own column mean) or 'zero'.  Every count defaults to 0 = off; no size is tuned.  Train graph only:
`evaluate`, every decoding algorithm and `align` never augment (csrc/specaugment.hip).
`video_augment` (None = off, or a dict; the reference only lists the intent, commented out, at the top of its resnet_cnn()) arrives
through **kwargs and augments the lip crops of `video_processing='resnet_cnn'` / `'3dconv_cnn'` inside the train step, anew every step
and the same for all frames of an utterance: `flip` (probability of a horizontal flip), `max_shift` (a shift of up to that many pixels
per axis, edges replicated), `contrast` (a factor 1 +- contrast about the utterance's own channel means), `brightness` (an offset of
+- brightness; no clipping).  Every value defaults to 0 = off; none is tuned.  Action-unit targets (`regress_aus`) are left as they are.
With `spec_augment` video time masks on as well, the masks fall on the augmented crops.  Train graph only, as above (INTEGRATION.md
section 8, csrc/video_augment.hip).
"""
import glob
import os
import time
from os import makedirs, path

import numpy as np
import torch

from . import ops
from .config import ModelConfig
from .io_utils import (_get_input_shape_from_record, create_unit_dict, make_iterator_from_one_record,
                       make_iterator_from_two_records)
from .model import Batch, Seq2SeqModel
from .parallel import DataParallelTrainer
from .utils import alignment_image, compute_wer, write_png_gray, write_sequences_to_labelfile


class AVSR(object):
    def __init__(self,
                 unit,
                 unit_file=None,
                 video_processing=None,
                 video_train_record=None,
                 video_test_record=None,
                 audio_processing=None,
                 audio_train_record=None,
                 audio_test_record=None,
                 labels_train_record=None,
                 labels_test_record=None,
                 batch_size=(64, 64),
                 cnn_filters=(8, 16, 32, 64),
                 cnn_dense_units=128,
                 regress_aus=False,
                 batch_normalisation=True,
                 instance_normalisation=False,
                 input_dense_layers=(0,),
                 architecture='unimodal',
                 encoder_type='unidirectional',
                 highway_encoder=False,
                 residual_encoder=False,
                 cell_type='lstm',
                 recurrent_l2_regularisation=0.0001,
                 weight_decay=0.0001,
                 encoder_units_per_layer=((256, ), (256, 256, 256)),
                 decoder_units_per_layer=(256,),
                 encoder_weight_sharing=False,
                 enable_attention=True,
                 attention_type=(('scaled_luong',)*1, ('scaled_luong',)*1),
                 use_dropout=True,
                 audio_encoder_dropout_probability=(0.9, 0.9, 0.9),
                 video_encoder_dropout_probability=(0.9, 0.9, 0.9),
                 decoder_dropout_probability=(0.9, 0.9, 0.9),
                 embedding_size=128,
                 sampling_probability_outputs=0.1,
                 label_smoothing=0.0,
                 decoding_algorithm='beam_search',
                 beam_width=10,
                 max_sentence_length=None,
                 optimiser='Adam',
                 learning_rate=0.001,
                 lr_decay=None,
                 loss_fun=None,
                 clip_gradients=True,
                 max_gradient_norm=1.0,
                 num_gpus=1,
                 write_attention_alignment=False,
                 write_beam_search_graphs=False,
                 write_estimated_modality_lags=False,
                 precision='float32',
                 profiling=False,
                 required_grahps=('train', 'eval'),
                 **kwargs):
        self._unit = unit
        self._unit_dict = create_unit_dict(unit_file=unit_file)
        self._video_processing, self._audio_processing = video_processing, audio_processing
        self._records = {
            'train': (video_train_record, audio_train_record, labels_train_record),
            'evaluate': (video_test_record, audio_test_record, labels_test_record)}
        self._batch_size = batch_size
        self._max_sentence_length = max_sentence_length
        self._required_graphs = required_grahps

        for name, val, ok in (("precision", precision, 'float32'),):
            if val != ok:
                raise NotImplementedError("%s=%r is a non-default option of the reference that the HIP engine does not build" % (name, val))
        self._profiling = bool(profiling)
        lr_decay_steps = 0
        if lr_decay is not None:                                                                  # seq2seq.py:263-273
            if lr_decay[0] == 'cosine_restarts':
                lr_decay_steps = int(lr_decay[1])
            else:
                print('learning rate policy not implemented, falling back to constant learning rate')
        if loss_fun not in (None, 'focal_loss', 'mc_loss'):
            raise ValueError('Unknown loss function {}'.format(loss_fun))                           # seq2seq.py:163
        if video_processing is not None and video_processing not in ('features', 'resnet_cnn', '3dconv_cnn'):
            if 'cnn' in video_processing:
                raise NotImplementedError("video_processing=%r: the `resnet_cnn` and `3dconv_cnn` front-ends are built" % video_processing)
            raise Exception('unknown visual content')                                             # avsr/avsr.py:713
        if audio_processing is not None and audio_processing not in ('features', 'wav'):
            raise NotImplementedError("audio_processing=%r: 'features' and 'wav' are built" % audio_processing)
        self._audio_frontend = None
        if audio_processing == 'wav':                     # raises here for the refused transformations / sample rates / filter counts
            from .audio_frontend import LogmelSpec
            self._audio_frontend = LogmelSpec(kwargs.get('audio_transformation', 'logmel_stack_w8s3'), kwargs.get('num_mel_bins', 30),
                                              kwargs.get('sample_rate', 16000))
        if decoding_algorithm not in ('greedy', 'beam_search', 'ctc_prefix_beam_search', 'attention_rescoring'):
            raise Exception('The only supported algorithms are `greedy`, `beam_search` and (not in the reference) '
                            '`ctc_prefix_beam_search`, `attention_rescoring`')                   # decoder_unimodal.py:124
        self._decoding_algorithm, self._beam_width = decoding_algorithm, beam_width
        if decoding_algorithm == 'ctc_prefix_beam_search':    # the CTC head's own search (csrc/ctc_prefix.hip): no decoder step at evaluate
            from ._lib import CTC_PREFIX_MAX_L, CTC_PREFIX_MAX_V, CTC_PREFIX_MAX_W
            if not kwargs.get('use_ctc', False):
                raise ValueError("decoding_algorithm='ctc_prefix_beam_search' needs use_ctc=True: the search runs on the CTC head")
            if len(self._unit_dict) - 1 > CTC_PREFIX_MAX_V or not 1 <= beam_width <= CTC_PREFIX_MAX_W:
                raise ValueError("decoding_algorithm='ctc_prefix_beam_search': avsr_ctc_prefix_search covers vocabularies of up to %d "
                                 "symbols and beam widths of 1 to %d (label sequences of up to %d; got %d symbols, beam_width %d)"
                                 % (CTC_PREFIX_MAX_V, CTC_PREFIX_MAX_W, CTC_PREFIX_MAX_L, len(self._unit_dict) - 1, beam_width))
        if decoding_algorithm == 'attention_rescoring':       # the prefix search's n-best rescored by the attention decoder (csrc/rescore.hip)
            from ._lib import CTC_PREFIX_MAX_L, CTC_PREFIX_MAX_V, CTC_PREFIX_MAX_W
            if not kwargs.get('use_ctc', False):
                raise ValueError("decoding_algorithm='attention_rescoring' needs use_ctc=True: the hypotheses are the CTC head's n-best")
            if len(self._unit_dict) - 1 > CTC_PREFIX_MAX_V or not 1 <= beam_width <= CTC_PREFIX_MAX_W:
                raise ValueError("decoding_algorithm='attention_rescoring': avsr_ctc_prefix_search covers vocabularies of up to %d "
                                 "symbols and beam widths of 1 to %d (label sequences of up to %d; got %d symbols, beam_width %d)"
                                 % (CTC_PREFIX_MAX_V, CTC_PREFIX_MAX_W, CTC_PREFIX_MAX_L, len(self._unit_dict) - 1, beam_width))
        self._write_attention_alignment = bool(write_attention_alignment)
        if self._write_attention_alignment and decoding_algorithm != 'greedy':
            raise NotImplementedError("write_attention_alignment=True needs decoding_algorithm='greedy' (the alignment history is "
                                      "kept by the greedy decode only)")

        # shallow-fusion language model: everything that can be refused is refused here, on the host, before any engine is built
        self._lm, self._lm_weight = None, float(kwargs.get('lm_weight', 0.3))
        lm_checkpoint, lm_cfg, lm_weights = kwargs.get('lm_checkpoint'), None, None
        if lm_checkpoint is not None:
            from . import lm as _lm                                 # (lm.py imports this module: bound late)
            if decoding_algorithm != 'beam_search':
                raise ValueError("lm_checkpoint needs decoding_algorithm='beam_search': the fusion is defined on the beam")
            lm_cfg = _lm.fusion_config(self._unit_dict, kwargs.get('lm_units_per_layer', (256,)), kwargs.get('lm_embedding_size', 128),
                                       kwargs.get('lm_cell_type', 'lstm'))
            lm_weights = _lm.checkpoint_weights(lm_cfg, lm_checkpoint)

        # back-off n-gram fused into beam search (csrc/beam_ngram.hip): parsed and compiled on the host, here, before any engine is built
        self._ngram = None
        ngram_lm = kwargs.get('ngram_lm')
        if ngram_lm is not None:
            from . import ngram as _ngram
            from ._lib import CTC_PREFIX_NGRAM_MAX_ARCS, CTC_PREFIX_NGRAM_MAX_NODES
            if decoding_algorithm != 'beam_search':
                raise ValueError("ngram_lm needs decoding_algorithm='beam_search': this keyword fuses the n-gram into the attention "
                                 "decoder's beam ('ctc_prefix_beam_search' takes ctc_ngram_lm; 'greedy' and 'attention_rescoring' take "
                                 "no language model)")
            if lm_checkpoint is not None:
                raise ValueError("ngram_lm and lm_checkpoint are two language models for one search: give one of them")
            if not self._lm_weight >= 0.0 or self._lm_weight == float('inf'):
                raise ValueError("lm_weight must be a finite number >= 0 (got %r)" % (kwargs.get('lm_weight'),))
            self._ngram = _ngram.load_tables(ngram_lm, self._unit_dict)             # ValueError: not an ARPA file, a token that is no unit
            if self._ngram["n_nodes"] > CTC_PREFIX_NGRAM_MAX_NODES or self._ngram["n_arcs"] > CTC_PREFIX_NGRAM_MAX_ARCS:
                raise ValueError("ngram_lm: avsr_beam_ngram_supported covers automata of up to %d nodes and %d arcs (got %d, %d)"
                                 % (CTC_PREFIX_NGRAM_MAX_NODES, CTC_PREFIX_NGRAM_MAX_ARCS, self._ngram["n_nodes"], self._ngram["n_arcs"]))

        # word-level n-gram behind a lexicon trie, fused into beam search (csrc/beam_word_ngram.hip): parsed, compiled and refused on the
        # host, here, before any engine is built; without the keyword nothing is read
        self._word_ngram = None
        word_ngram_lm = kwargs.get('word_ngram_lm')
        if word_ngram_lm is not None:
            from . import ngram as _ngram
            from ._lib import CTC_PREFIX_NGRAM_MAX_ARCS, CTC_PREFIX_NGRAM_MAX_NODES
            if decoding_algorithm != 'beam_search':
                raise ValueError("word_ngram_lm needs decoding_algorithm='beam_search': this keyword fuses the word model into the "
                                 "attention decoder's beam ('ctc_prefix_beam_search' takes ctc_word_ngram_lm; 'greedy' and "
                                 "'attention_rescoring' take no language model)")
            if lm_checkpoint is not None or ngram_lm is not None:
                raise ValueError("word_ngram_lm and %s are two language models for one search: give one of them"
                                 % ("lm_checkpoint" if lm_checkpoint is not None else "ngram_lm"))
            if not self._lm_weight >= 0.0 or self._lm_weight == float('inf'):
                raise ValueError("lm_weight must be a finite number >= 0 (got %r)" % (kwargs.get('lm_weight'),))
            # ValueError: not an ARPA file, units that cannot spell (no ' ', multi-character units), no spellable word, a bad oov score
            g = self._word_ngram = _ngram.load_word_tables(word_ngram_lm, self._unit_dict, kwargs.get('word_oov_score', -10.0))
            if max(g["n_nodes"], g["n_trie_nodes"]) > CTC_PREFIX_NGRAM_MAX_NODES or max(g["n_arcs"], g["n_trie_arcs"]) > CTC_PREFIX_NGRAM_MAX_ARCS:
                raise ValueError("word_ngram_lm: avsr_beam_word_ngram_supported covers word automata and lexicon tries of up to %d nodes "
                                 "and %d arcs each (got %d, %d and %d, %d)"
                                 % (CTC_PREFIX_NGRAM_MAX_NODES, CTC_PREFIX_NGRAM_MAX_ARCS, g["n_nodes"], g["n_arcs"], g["n_trie_nodes"],
                                    g["n_trie_arcs"]))

        # language model fused into the CTC prefix search (csrc/ctc_prefix_lm.hip): its own keywords, refused on the host like lm_checkpoint
        self._ctc_lm = None
        self._ctc_lm_weight, self._ctc_lm_bonus = float(kwargs.get('ctc_lm_weight', 0.3)), float(kwargs.get('ctc_lm_length_bonus', 0.0))
        if not self._ctc_lm_weight >= 0.0 or self._ctc_lm_weight == float('inf'):
            raise ValueError("ctc_lm_weight must be a finite number >= 0 (got %r)" % (kwargs.get('ctc_lm_weight'),))
        if self._ctc_lm_bonus != self._ctc_lm_bonus or abs(self._ctc_lm_bonus) == float('inf'):
            raise ValueError("ctc_lm_length_bonus must be finite (got %r)" % (kwargs.get('ctc_lm_length_bonus'),))
        ctc_lm_checkpoint, ctc_lm_cfg, ctc_lm_weights = kwargs.get('ctc_lm_checkpoint'), None, None
        if ctc_lm_checkpoint is not None:
            from . import lm as _lm
            from ._lib import CTC_PREFIX_LM_MAX_W, MAX_LM_LAYERS
            if decoding_algorithm != 'ctc_prefix_beam_search':
                raise ValueError("ctc_lm_checkpoint needs decoding_algorithm='ctc_prefix_beam_search': the model is fused into the CTC "
                                 "head's own search (beam search takes lm_checkpoint; 'attention_rescoring' takes no language model)")
            ctc_lm_cfg = _lm.fusion_config(self._unit_dict, kwargs.get('lm_units_per_layer', (256,)), kwargs.get('lm_embedding_size', 128),
                                           kwargs.get('lm_cell_type', 'lstm'))
            if beam_width > CTC_PREFIX_LM_MAX_W or len(ctc_lm_cfg.decoder_units) > MAX_LM_LAYERS:
                raise ValueError("ctc_lm_checkpoint: avsr_ctc_prefix_lm_supported covers beam widths of up to %d and language models of up "
                                 "to %d layers (got beam_width %d, %d layers)"
                                 % (CTC_PREFIX_LM_MAX_W, MAX_LM_LAYERS, beam_width, len(ctc_lm_cfg.decoder_units)))
            ctc_lm_weights = _lm.checkpoint_weights(ctc_lm_cfg, ctc_lm_checkpoint)

        # back-off n-gram fused into the CTC prefix search (csrc/ctc_prefix_ngram.hip): parsed and compiled on the host, here
        self._ctc_ngram = None
        ctc_ngram_lm = kwargs.get('ctc_ngram_lm')
        if ctc_ngram_lm is not None:
            from . import ngram as _ngram
            from ._lib import CTC_PREFIX_LM_MAX_W
            if decoding_algorithm != 'ctc_prefix_beam_search':
                raise ValueError("ctc_ngram_lm needs decoding_algorithm='ctc_prefix_beam_search': the n-gram is fused into the CTC head's "
                                 "own search ('beam_search' takes ngram_lm; 'attention_rescoring' takes no n-gram)")
            if ctc_lm_checkpoint is not None:
                raise ValueError("ctc_ngram_lm and ctc_lm_checkpoint are two language models for one search: give one of them")
            if beam_width > CTC_PREFIX_LM_MAX_W:
                raise ValueError("ctc_ngram_lm: avsr_ctc_prefix_ngram_supported covers beam widths of up to %d (got beam_width %d)"
                                 % (CTC_PREFIX_LM_MAX_W, beam_width))
            self._ctc_ngram = _ngram.load_tables(ctc_ngram_lm, self._unit_dict)     # ValueError: not an ARPA file, a token that is no unit
            from ._lib import CTC_PREFIX_NGRAM_MAX_NODES, CTC_PREFIX_NGRAM_MAX_ARCS
            if self._ctc_ngram["n_nodes"] > CTC_PREFIX_NGRAM_MAX_NODES or self._ctc_ngram["n_arcs"] > CTC_PREFIX_NGRAM_MAX_ARCS:
                raise ValueError("ctc_ngram_lm: avsr_ctc_prefix_ngram_supported covers automata of up to %d nodes and %d arcs (got %d, %d)"
                                 % (CTC_PREFIX_NGRAM_MAX_NODES, CTC_PREFIX_NGRAM_MAX_ARCS, self._ctc_ngram["n_nodes"],
                                    self._ctc_ngram["n_arcs"]))

        # word-level n-gram behind a lexicon trie, fused into the CTC prefix search (csrc/ctc_prefix_word_ngram.hip): parsed, compiled and
        # refused on the host, here; without the keyword nothing is read
        self._ctc_word_ngram = None
        ctc_word_ngram_lm = kwargs.get('ctc_word_ngram_lm')
        if ctc_word_ngram_lm is not None:
            from . import ngram as _ngram
            from ._lib import CTC_PREFIX_LM_MAX_W, CTC_PREFIX_NGRAM_MAX_ARCS, CTC_PREFIX_NGRAM_MAX_NODES
            if decoding_algorithm != 'ctc_prefix_beam_search':
                raise ValueError("ctc_word_ngram_lm needs decoding_algorithm='ctc_prefix_beam_search': the word model is fused into the "
                                 "CTC head's own search ('beam_search' takes word_ngram_lm; 'greedy' and 'attention_rescoring' take no word-level "
                                 "model)")
            if ctc_lm_checkpoint is not None or ctc_ngram_lm is not None:
                raise ValueError("ctc_word_ngram_lm and %s are two language models for one search: give one of them"
                                 % ("ctc_lm_checkpoint" if ctc_lm_checkpoint is not None else "ctc_ngram_lm"))
            if beam_width > CTC_PREFIX_LM_MAX_W:
                raise ValueError("ctc_word_ngram_lm: avsr_ctc_prefix_word_ngram_supported covers beam widths of up to %d (got beam_width "
                                 "%d)" % (CTC_PREFIX_LM_MAX_W, beam_width))
            # ValueError: not an ARPA file, units that cannot spell (no ' ', multi-character units), no spellable word, a bad oov score
            g = self._ctc_word_ngram = _ngram.load_word_tables(ctc_word_ngram_lm, self._unit_dict, kwargs.get('ctc_word_oov_score', -10.0))
            if max(g["n_nodes"], g["n_trie_nodes"]) > CTC_PREFIX_NGRAM_MAX_NODES or max(g["n_arcs"], g["n_trie_arcs"]) > CTC_PREFIX_NGRAM_MAX_ARCS:
                raise ValueError("ctc_word_ngram_lm: avsr_ctc_prefix_word_ngram_supported covers word automata and lexicon tries of up to "
                                 "%d nodes and %d arcs each (got %d, %d and %d, %d)"
                                 % (CTC_PREFIX_NGRAM_MAX_NODES, CTC_PREFIX_NGRAM_MAX_ARCS, g["n_nodes"], g["n_arcs"], g["n_trie_nodes"],
                                    g["n_trie_arcs"]))

        # joint CTC / attention scoring in beam search: an evaluate-time weight, held like _lm_weight; 0 = off, nothing new is launched
        self._ctc_decode_weight = float(kwargs.get('ctc_decode_weight', 0.0))
        if not self._ctc_decode_weight >= 0.0 or self._ctc_decode_weight == float('inf'):
            raise ValueError("ctc_decode_weight must be a finite number >= 0 (got %r)" % (kwargs.get('ctc_decode_weight'),))
        if self._ctc_decode_weight != 0.0:
            from ._lib import BEAM_CTC_MAX_V
            if not kwargs.get('use_ctc', False):
                raise ValueError("ctc_decode_weight needs use_ctc=True: the term is the CTC head's prefix score")
            if decoding_algorithm not in ('beam_search', 'attention_rescoring'):
                raise ValueError("ctc_decode_weight needs decoding_algorithm='beam_search' (the joint scoring is defined on the beam) "
                                 "or 'attention_rescoring' (the weight of the n-best's CTC score)")
            if decoding_algorithm == 'beam_search' and (len(self._unit_dict) - 1 > BEAM_CTC_MAX_V or beam_width > 64):
                raise ValueError("ctc_decode_weight: avsr_beam_ctc_supported covers vocabularies of up to %d symbols and beam widths "
                                 "of up to 64 (got %d, %d)" % (BEAM_CTC_MAX_V, len(self._unit_dict) - 1, beam_width))

        reverse = {v: k for k, v in self._unit_dict.items()}
        feats, video_hw = {}, (36, 36, 3)
        for idx, (proc, key) in enumerate(((video_processing, 'video'), (audio_processing, 'audio'))):
            rec = self._records['train'][idx] or self._records['evaluate'][idx]
            if proc is not None:
                shape, _ = _get_input_shape_from_record(rec)
                if key == 'video' and proc in ('resnet_cnn', '3dconv_cnn'):
                    if len(shape) != 3:
                        raise ValueError("video_processing=%r needs raw [width, height, channels] frames in the video record" % proc)
                    video_hw, feats[key] = tuple(shape), cnn_dense_units
                    continue
                if len(shape) != 1:
                    raise ValueError("raw video records need video_processing='resnet_cnn' or '3dconv_cnn'")
                if key == 'audio' and proc == 'wav':
                    if shape[0] != 1:
                        raise ValueError("audio_processing='wav' needs a waveform record (input_size == 1), got input_size == %d" % shape[0])
                    feats[key] = self._audio_frontend.feat
                    continue
                feats[key] = shape[0]
        # SpecAugment in the train step (csrc/specaugment.hip): parsed and refused here, on the host, before any engine is built
        from .config import spec_augment_fields
        spec_fields = spec_augment_fields(kwargs.get('spec_augment'), audio=audio_processing is not None, video=video_processing is not None,
                                          audio_processing=audio_processing, audio_feat=feats.get('audio'),
                                          num_mel_bins=kwargs.get('num_mel_bins', 30))
        # lip-crop augmentation in the train step (csrc/video_augment.hip): likewise
        from .config import video_augment_fields
        spec_fields.update(video_augment_fields(kwargs.get('video_augment'), video_processing, video_hw))
        self._cfg = ModelConfig(
            **spec_fields,
            architecture=architecture, encoder_type=encoder_type, cell_type=cell_type,
            video_units=tuple(encoder_units_per_layer[0]) if video_processing is not None else None,
            audio_units=tuple(encoder_units_per_layer[1]) if audio_processing is not None else None,
            decoder_units=tuple(decoder_units_per_layer), attention_type=tuple(tuple(t) for t in attention_type),
            enable_attention=enable_attention, embedding_size=embedding_size,
            vocab_size=len(self._unit_dict) - 1, go_id=reverse['GO'], eos_id=reverse['EOS'],
            video_feat=feats.get('video', 128), audio_feat=feats.get('audio', 80),
            batch_normalisation=batch_normalisation, regress_aus=regress_aus,
            au_loss_weight=kwargs.get('au_loss_weight', 10.0),
            use_ctc=bool(kwargs.get('use_ctc', False)), ctc_weight=float(kwargs.get('ctc_weight', 0.3)),
            recurrent_l2=None if optimiser == 'AdamW' else recurrent_l2_regularisation,     # avsr.py:168
            optimiser=optimiser, weight_decay=weight_decay, clip_gradients=clip_gradients, max_gradient_norm=max_gradient_norm,
            learning_rate=learning_rate, warmup_steps=kwargs.get('warmup_steps', 750), lr_decay_steps=lr_decay_steps, loss_fun=loss_fun, label_smoothing=float(label_smoothing),
            max_label_length={'viseme': 150, 'phoneme': 150, 'character': 150}[unit],
            use_dropout=use_dropout, video_dropout=tuple(video_encoder_dropout_probability),
            audio_dropout=tuple(audio_encoder_dropout_probability), decoder_dropout=tuple(decoder_dropout_probability),
            sampling_probability=sampling_probability_outputs,
            video_processing=video_processing if video_processing is not None else 'features',
            audio_processing=audio_processing if audio_processing is not None else 'features',
            **({} if self._audio_frontend is None else dict(zip(('audio_transformation', 'num_mel_bins', 'sample_rate'),
                                                                 self._audio_frontend.key()))),
            cnn_filters=tuple(cnn_filters), cnn_dense_units=cnn_dense_units, video_hw=video_hw,
            input_dense_layers=tuple(input_dense_layers), encoder_weight_sharing=bool(encoder_weight_sharing), residual_encoder=bool(residual_encoder), highway_encoder=bool(highway_encoder), instance_normalisation=bool(instance_normalisation))
        self._model = Seq2SeqModel(self._cfg, seed=kwargs.get('seed', 0))
        if lm_cfg is not None:
            self._lm = _lm.load_fusion_engine(lm_cfg, lm_weights)
        if ctc_lm_cfg is not None:
            self._ctc_lm = _lm.load_fusion_engine(ctc_lm_cfg, ctc_lm_weights)
        self._shuffle_seed = kwargs.get('shuffle_seed')        # None = a fresh order every run, as tf.data's unseeded shuffle(5000)
        # Data parallelism (the reference's num_gpus is deprecated and ignored, avsr/avsr.py:67,:127): when the process was started
        # under torch.distributed (one process per GPU, `torchrun`), every rank builds the same model, reads the same records,
        # shards each bucketed batch by utterance and all-reduces normalisers / BN statistics / gradients over RCCL (parallel.py).
        import torch.distributed as _dist
        self._epoch_counter = 0
        self._dist = _dist if (_dist.is_available() and _dist.is_initialized() and _dist.get_world_size() > 1) else None
        self._rank = self._dist.get_rank() if self._dist is not None else 0
        self._world = self._dist.get_world_size() if self._dist is not None else 1
        if self._dist is not None and self._shuffle_seed is None:      # every rank must draw the same shuffle order
            seed_t = torch.randint(0, 2 ** 31 - 1, (1,), dtype=torch.int64)
            if _dist.get_backend() == 'nccl':
                seed_t = seed_t.cuda()
            _dist.broadcast(seed_t, src=0)
            self._shuffle_seed = int(seed_t.item())
        # bucketed batches: shapes vary per step, but full buckets at the longest lengths come back -- a shape is captured into a hipGraph
        # at its second sighting and replayed from then on (AVSR_TRAIN_GRAPH=0: eager launches only)
        # (profiling=True brackets every launch with an event pair: eager launches)
        self._trainer = DataParallelTrainer(self._model, self._dist,
                                            use_graph=os.environ.get("AVSR_TRAIN_GRAPH", "1") != "0" and not self._profiling,
                                            check_every_step=True, graph_after=2,
                                            # every captured shape pins its workspace (lip-CNN activations: GBs at B = 64) next to the
                                            # 8 unpinned ones of the model's LRU: keep few
                                            max_graphs=int(os.environ.get("AVSR_TRAIN_MAX_GRAPHS", "8")))

    # ------------------------------------------------------------------------------------------------
    def _iterator(self, mode):
        vrec, arec, lrec = self._records[mode]
        bs = self._batch_size[0 if mode == 'train' else 1]
        shuffle = mode == 'train'
        # training batches are sharded by utterance across the data-parallel ranks; evaluation runs whole on every rank
        rank, world = (self._rank, self._world) if mode == 'train' else (0, 1)
        seed = self._shuffle_seed
        if seed is not None:
            seed = seed + self._epoch_counter                     # a new order every epoch; under data parallelism identical on every rank
        if self._video_processing is not None and self._audio_processing is not None:
            return make_iterator_from_two_records(vrec, arec, lrec, bs, self._unit_dict, shuffle=shuffle, bucket_width=45,
                                                  seed=seed, rank=rank, world=world, audio_frontend=self._audio_frontend)
        rec = vrec if self._video_processing is not None else arec
        return make_iterator_from_one_record(rec, lrec, self._unit_dict, bs, shuffle=shuffle, bucket_width=45,
                                             max_sentence_length=self._max_sentence_length if self._audio_processing is not None else None,
                                             seed=seed, rank=rank, world=world,
                                             audio_frontend=self._audio_frontend if self._audio_processing is not None else None)

    @staticmethod
    def _prefetched(it, depth=2):
        """Batches of `it`, produced by a helper thread up to `depth` ahead: TFRecord indexing and the padding copies (ctypes calls into
        libavsr_io.so, which release the GIL) run while the launching thread waits for the GPU step -- with the step replayed from a
        hipGraph that thread is idle almost all of the time.  depth + 3 <= the pipeline's buffer ring (io_utils._Pipeline.RING): `depth` queued, one being filled, two held by the training
        loop (the step in flight and the batch whose upload overlaps it)."""
        import queue
        import threading
        q, end = queue.Queue(maxsize=depth), object()
        dev = torch.cuda.current_device() if torch.cuda.is_available() else None

        def run():
            try:
                if dev is not None:
                    torch.cuda.set_device(dev)            # page-locked buffers are allocated here: on THIS rank's device, not on device 0
                for b in it:
                    q.put(b)
                q.put(end)
            except BaseException as e:                        # surfaces in the consumer
                q.put(e)

        threading.Thread(target=run, daemon=True).start()
        while True:
            x = q.get()
            if x is end:
                return
            if isinstance(x, BaseException):
                raise x
            yield x

    def _to_batch(self, bd):
        # (non_blocking: the big input arrays of a training batch live in page-locked ring buffers -- an asynchronous DMA, stream-ordered
        # ahead of the step's kernels; for pageable arrays the flag changes nothing)
        t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda(non_blocking=True)
        b = Batch(labels=t(bd.labels, torch.int32), labels_len=t(bd.labels_length, torch.int32))
        if isinstance(bd.inputs, tuple):
            b.video, b.audio = t(bd.inputs[0], torch.float32), t(bd.inputs[1], torch.float32)
            b.video_len, b.audio_len = t(bd.inputs_length[0], torch.int32), t(bd.inputs_length[1], torch.int32)
            names = bd.inputs_filenames[0]
        elif self._video_processing is not None:
            b.video, b.video_len, names = t(bd.inputs, torch.float32), t(bd.inputs_length, torch.int32), bd.inputs_filenames
        else:
            b.audio, b.audio_len, names = t(bd.inputs, torch.float32), t(bd.inputs_length, torch.int32), bd.inputs_filenames
        if 'aus' in bd.payload:
            b.aus = t(bd.payload['aus'], torch.float32)
        elif self._cfg.regress_aus and b.video is not None:
            raise ValueError("regress_aus=True needs Action Units in the video record")
        return b, names

    # ------------------------------------------------------------------------------------------------
    def save(self, checkpoint_path):
        m = self._model
        blob = {"step": np.array(int(m.step.item()), np.int64)}
        for which in ("params", "adam_m", "adam_v"):
            for k, v in m.export_tf_weights(which).items():
                blob[which + ":" + k] = v
        fe = getattr(self, "_audio_frontend", None)       # (avsr.LM borrows save / restore and has no front-end)
        if fe is not None:                                # the front-end has no variables: its configuration is the checkpoint's metadata
            blob["meta:audio_frontend"] = np.array([str(v) for v in fe.key()])
        makedirs(path.dirname(checkpoint_path), exist_ok=True)
        np.savez(checkpoint_path + ".npz", **blob)
        return checkpoint_path

    def restore(self, checkpoint_path):
        z = np.load(checkpoint_path if checkpoint_path.endswith(".npz") else checkpoint_path + ".npz")
        m = self._model
        fe = getattr(self, "_audio_frontend", None)
        if "meta:audio_frontend" in z.files and fe is not None:
            saved, mine = [str(v) for v in z["meta:audio_frontend"]], [str(v) for v in fe.key()]
            if saved != mine:
                raise ValueError("checkpoint was trained with the audio front-end %s, this model has %s" % (saved, mine))
        m.load_tf_weights({k[7:]: z[k] for k in z.files if k.startswith("params:")})
        for which, buf in (("adam_m", m.adam_m), ("adam_v", m.adam_v)):
            W = {k[len(which) + 1:]: z[k] for k in z.files if k.startswith(which + ":")}
            if W:
                m.load_flat(buf, W)
        m.step.fill_(int(z["step"]))

    @staticmethod
    def latest_checkpoint(checkpoint_dir):
        files = glob.glob(path.join(checkpoint_dir, "checkpoint.ckp-*.npz"))
        if not files:
            return None
        best = max(files, key=lambda f: int(f[:-4].split('-')[-1]))
        return best[:-4]

    # ------------------------------------------------------------------------------------------------
    def train(self, logfile, num_epochs=400, try_restore_latest_checkpoint=False):
        checkpoint_dir = path.join('checkpoints', path.split(logfile)[-1])
        checkpoint_path = path.join(checkpoint_dir, 'checkpoint.ckp')
        makedirs(checkpoint_dir, exist_ok=True)
        if path.dirname(logfile):
            makedirs(path.dirname(logfile), exist_ok=True)
        last_epoch = 0
        if try_restore_latest_checkpoint is True:
            try:
                latest_ckp = self.latest_checkpoint(checkpoint_dir)
                last_epoch = int(latest_ckp.split('-')[-1])
                self.restore(latest_ckp)
                print('Restoring checkpoint from epoch {}\n'.format(last_epoch))
            except Exception:
                print('Could not restore from checkpoint, training from scratch!\n')
        lead = self._rank == 0                                  # side-effect files (log, checkpoints, predictions) are written by rank 0
        f = open(logfile if lead else os.devnull, 'a')
        for current_epoch in range(1, num_epochs):            # num_epochs - 1 epochs actually run (avsr.py:253)
            epoch = last_epoch + current_epoch
            self._epoch_counter = epoch
            sum_loss, batches = 0.0, 0
            start = time.time()
            it = self._iterator('train')
            if hasattr(it, "reuse_buffers") and os.environ.get("AVSR_IO_PREFETCH", "1") != "0":
                it.reuse_buffers = True                       # each batch is consumed (copied to the device) before the one after next is asked for
                it = self._prefetched(it, depth=2)            # (+ 2 batches held by the loop below: RING >= 5)
            # The NEXT batch's host-to-device copy (85 MB of lip crops + audio at the benchmark shape: ~1.5 ms of PCIe) runs on a copy
            # stream while the current step computes: it is started before the step is launched (the trainer waits for the GPU inside
            # train_step when it checks the persistent kernels' flag).
            it = iter(it)
            copy_stream = torch.cuda.Stream()

            def upload(bd):
                if bd is None:
                    return None
                with torch.cuda.stream(copy_stream):
                    batch, _names = self._to_batch(bd)
                    ev = torch.cuda.Event()
                    ev.record(copy_stream)
                return batch, ev

            nxt = upload(next(it, None))
            while nxt is not None:                            # end of data = StopIteration (reference: OutOfRangeError)
                batch, ev = nxt
                cur = torch.cuda.current_stream()
                cur.wait_event(ev)
                for t_ in vars(batch).values():               # allocated on the copy stream, consumed on this one
                    if torch.is_tensor(t_):
                        t_.record_stream(cur)
                nxt = upload(next(it, None))                  # (the prefetch thread is normally ahead: no wait here)
                if self._profiling:
                    ops.prof_begin(1 << 16)
                loss, gnorm = self._trainer.train_step(batch)
                if self._profiling:
                    self._write_timeline(ops.prof_end(), epoch, batches)
                batch_loss, global_norm = float(loss.item()), float(gnorm.item())
                sum_loss += batch_loss
                if lead:
                    print('batch: {}, batch loss: {:.2f}, gradient norm: {:.2f}'.format(batches, batch_loss, global_norm))
                batches += 1
            if lead:
                print('epoch time: {}'.format(time.time() - start))
            f.write('Average batch_loss as epoch {} is {}\n'.format(epoch, sum_loss / max(1, batches)))
            f.flush()
            if epoch % 10 == 0:
                save_path = checkpoint_path + '-{}'.format(epoch)
                if lead:
                    self.save(save_path)
                if self._dist is not None:
                    self._dist.barrier()                          # the other ranks restore the file rank 0 has just written
                error_rate = self.evaluate(save_path, epoch)
                for (k, v) in error_rate.items():
                    f.write(k + ': {:.4f}% '.format(v * 100))
                f.write('\n')
                f.flush()
        f.close()

    @staticmethod
    def _write_timeline(prof, epoch, batch):
        """`profiling=True` (avsr/avsr.py:542-550, :274-290 drive tf.profiler with FULL_TRACE and write timelines to /tmp/timelines/):
        here every engine launch of the step is bracketed by a HIP event pair (avsr_prof_begin / avsr_prof_end) and the per-kernel-
        class launch counts, summed milliseconds and algorithmic FLOPs of the step go to /tmp/timelines/timeline_<epoch>_<batch>.json.
        For a kernel-by-kernel trace run the same script under `rocprofv3 --kernel-trace --stats`."""
        import json
        makedirs('/tmp/timelines/', exist_ok=True)
        rows = {k: {"launches": c, "ms": round(ms, 4), "algorithmic_gflop": round(fl / 1e9, 3)} for k, (c, ms, fl) in prof.items() if c}
        with open('/tmp/timelines/timeline_{}_{}.json'.format(epoch, batch), 'w') as f:
            json.dump({"epoch": epoch, "batch": batch, "kernel_classes": rows, "total_ms": round(sum(r["ms"] for r in rows.values()), 4)}, f, indent=1)

    def _write_alignments(self, names, alignments_outdir):
        """`<file>.png` (unimodal / av_align decoder), `<file>_video.png` + `<file>_audio.png` (bimodal), `<file>_av.png`
        (AV-Align cross-modal), one greyscale image [T_memory x T_decoder] per utterance (avsr/avsr.py:404-436)."""
        al = self._model.attention_alignments()
        dec = [a.cpu().numpy() for a in al["decoder"]]
        enc = None if al["encoder"] is None else al["encoder"].cpu().numpy()
        arch = self._cfg.architecture
        for idx in range(len(names)):
            base = path.join(alignments_outdir, names[idx].decode('utf-8'))
            makedirs(path.dirname(base), exist_ok=True)
            if arch == 'bimodal':
                write_png_gray(base + '_video.png', alignment_image(dec[0][idx]))
                write_png_gray(base + '_audio.png', alignment_image(dec[-1][idx]))
            else:
                write_png_gray(base + '.png', alignment_image(dec[0][idx]))
                if arch == 'av_align':
                    write_png_gray(base + '_av.png', alignment_image(enc[idx]))

    def _decode(self, batch):
        """The predictions of one batch under `decoding_algorithm`: rows of ids (a numpy array or a list of id lists)."""
        if self._decoding_algorithm == 'beam_search':     # avsr.py:58-59 default: width 10, first beam returned
            fused = self._lm is not None or self._ngram is not None or self._word_ngram is not None
            ids = self._model.beam_search_decode(batch, beam_width=self._beam_width, max_steps=self._cfg.max_label_length,
                                                 lm=self._lm, ngram=self._ngram,
                                                 lm_weight=self._lm_weight if fused else 0.0,
                                                 **({} if self._word_ngram is None else dict(word_ngram=self._word_ngram)),
                                                 ctc_weight=self._ctc_decode_weight)
        elif self._decoding_algorithm == 'attention_rescoring':        # two passes: the head's n-best, then teacher-forced scoring
            ids = self._model.attention_rescoring(batch, beam_width=self._beam_width, max_steps=self._cfg.max_label_length,
                                                  ctc_weight=self._ctc_decode_weight)
        elif self._decoding_algorithm == 'ctc_prefix_beam_search':     # the head's own search: the attention decoder never runs
            ids = self._model.ctc_prefix_beam_search(batch, beam_width=self._beam_width, max_steps=self._cfg.max_label_length,
                                                     lm=self._ctc_lm, lm_weight=self._ctc_lm_weight, length_bonus=self._ctc_lm_bonus,
                                                     ngram=self._ctc_ngram,
                                                     **({} if self._ctc_word_ngram is None else dict(word_ngram=self._ctc_word_ngram)))
        else:
            ids = self._model.greedy_decode(batch, max_steps=self._cfg.max_label_length)
        if not isinstance(ids, list):
            ids = ids.cpu().numpy()
        return ids

    def align(self, checkpoint_path, epoch=None, targets='labels', frame_shift=None):
        """Forced alignment on the CTC head (not in the reference; INTEGRATION.md section 8, csrc/ctc_align.hip): restores the checkpoint,
        walks the evaluate records and returns {name: [(symbol, start, end, confidence), ...]}, one tuple per label -- the Viterbi
        alignment of each utterance's labels (targets='labels', the EOS left out) or of what `evaluate` would predict for it
        (targets='predictions', cut at the first EOS).  start / end are the first / last frame of the label's run, frames of the CTC
        stream's encoder; with frame_shift (seconds per frame, the caller's knowledge of the features) they are seconds rounded to three
        decimals and end is exclusive.  confidence = exp(mean log-probability of the run's frames).  An utterance whose target has no
        valid alignment (fewer frames than labels plus adjacent repeats) maps to None.  Rank 0 writes
        predictions/<run>/ctc_alignment_epoch_<N>.txt: per utterance `name score`, one `start end symbol confidence` line per label
        (or `# no alignment`), then a line holding `.`."""
        if not self._cfg.use_ctc:
            raise ValueError("align needs use_ctc=True: the alignment is computed on the CTC head")
        if targets not in ('labels', 'predictions'):
            raise ValueError("align: targets must be 'labels' or 'predictions' (got %r)" % (targets,))
        if frame_shift is not None and not (float(frame_shift) > 0.0 and float(frame_shift) < float('inf')):
            raise ValueError("align: frame_shift must be a positive number of seconds per frame (got %r)" % (frame_shift,))
        self.restore(checkpoint_path)
        eos = self._cfg.eos_id
        result, scores = {}, {}
        for bd in self._iterator('evaluate'):
            batch, names = self._to_batch(bd)
            tg = None
            if targets == 'predictions':
                tg = []
                for row in self._decode(batch):
                    row = [int(s) for s in row]
                    tg.append(row[:row.index(eos)] if eos in row else row)
            for name, al in zip(names, self._model.ctc_align(batch, tg)):
                file = name.decode('utf-8')
                scores[file] = al['score']
                if not al['status']:
                    result[file] = None
                    continue
                segs = []
                for lab, s, e, conf in al['segments']:
                    if frame_shift is not None:
                        s, e = round(s * float(frame_shift), 3), round((e + 1) * float(frame_shift), 3)
                    segs.append((self._unit_dict[lab], s, e, conf))
                result[file] = segs
        if self._rank == 0:
            outdir = path.join('predictions', path.split(path.split(checkpoint_path)[0])[-1])
            makedirs(outdir, exist_ok=True)
            tf = '{:.3f}' if frame_shift is not None else '{:d}'
            with open(path.join(outdir, 'ctc_alignment_epoch_{}.txt'.format(epoch)), 'w') as f:
                for file, segs in result.items():
                    f.write('{} {:.6f}\n'.format(file, scores[file]))
                    if segs is None:
                        f.write('# no alignment\n')
                    for sym, s, e, conf in segs or ():
                        f.write((tf + ' ' + tf + ' {} {:.6f}\n').format(s, e, sym, conf))
                    f.write('.\n')
        return result

    def evaluate(self, checkpoint_path, epoch=None, alignments_outdir='./alignments/tmp/', beam_graphs_outdir='./beam_graphs/tmp/'):
        self.restore(checkpoint_path)                         # the path argument is honoured, as in avsr.py:328-331
        predictions_dict, labels_dict, ctc_dict = {}, {}, {}
        it = self._iterator('evaluate')
        if hasattr(it, "reuse_buffers") and os.environ.get("AVSR_IO_PREFETCH", "1") != "0":
            it.reuse_buffers = True                       # a batch is decoded (host-synchronised) before the next one is asked for
            it = self._prefetched(it, depth=2)
        for bd in it:
            batch, names = self._to_batch(bd)
            ids = self._decode(batch)
            if self._write_attention_alignment:
                self._write_alignments(names, alignments_outdir)
            for idx in range(len(names)):
                file = names[idx].decode('utf-8')
                predictions_dict[file] = [self._unit_dict[int(s)] for s in ids[idx]]
                labels_dict[file] = [self._unit_dict[int(s)] for s in bd.labels[idx]]
            if self._cfg.use_ctc:                             # the CTC head's best path, scored like the decoder's output
                for idx, seq in enumerate(self._model.ctc_best_path(batch)):
                    ctc_dict[names[idx].decode('utf-8')] = [self._unit_dict[s] for s in seq]
        uer, uer_dict = compute_wer(predictions_dict, labels_dict)
        error_rate = {self._unit: uer}
        if self._unit == 'character':
            wer, _wer_dict = compute_wer(predictions_dict, labels_dict, split_words=True)
            error_rate['word'] = wer
        if self._cfg.use_ctc:
            error_rate['ctc_' + self._unit], _ctc_uer_dict = compute_wer(ctc_dict, labels_dict)
        if self._rank == 0:
            outdir = path.join('predictions', path.split(path.split(checkpoint_path)[0])[-1])
            makedirs(outdir, exist_ok=True)
            write_sequences_to_labelfile(predictions_dict, path.join(outdir, 'predicted_epoch_{}.mlf'.format(epoch)), labels_dict,
                                         uer_dict, sep=' ' if self._unit == 'phoneme' else '')
        return error_rate
