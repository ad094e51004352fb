"""Hyper-parameters the hot path reads (mirror of the HParams bag, avsr/avsr.py:150-198)."""
from dataclasses import dataclass, replace
from typing import List, Optional, Tuple

LUONG_TYPES = ("luong", "scaled_luong")
BAHDANAU_TYPES = ("bahdanau", "normed_bahdanau")
ATT_CODE = {"luong": 0, "scaled_luong": 1, "bahdanau": 2, "normed_bahdanau": 3}
CELL_ID_DECODER = 40
# RNG streams of the SpecAugment draws (csrc/common.h RNG_STREAM_SPEC_*): above every dropout / sampling stream, which are
# cell_id * 4 + kind with cell ids up to CELL_ID_DECODER + 3 (a four-layer decoder)
SPEC_STREAM_AUDIO_FREQ, SPEC_STREAM_AUDIO_TIME, SPEC_STREAM_VIDEO_TIME = 200, 201, 202
SPEC_AUGMENT_KEYS = ("freq_masks", "freq_width", "time_masks", "time_width", "time_ratio", "video_time_masks", "video_time_width",
                     "video_time_ratio", "freq_bins", "mask_value")
SPEC_AUGMENT_MAX_MASKS, SPEC_AUGMENT_MAX_T = 8, 65535          # avsr_spec_augment_supported (include/avsr_hip.h)
# ... and of the lip-crop augmentation's draws (csrc/common.h RNG_STREAM_VIDEO_AUG_*): flip and shifts; contrast and brightness
VIDEO_AUG_STREAM_GEOMETRY, VIDEO_AUG_STREAM_PHOTOMETRIC = 203, 204
VIDEO_AUGMENT_KEYS = ("flip", "max_shift", "contrast", "brightness")


def round4(n: int) -> int:
    return (n + 3) // 4 * 4


def spec_augment_fields(spec, audio=True, video=True, audio_processing="features", audio_feat=None, num_mel_bins=30):
    """The `spec_augment` keyword of avsr.AVSR (None, or a dict over SPEC_AUGMENT_KEYS) -> the ModelConfig fields it sets.  Refuses on
    the host, naming the key (ValueError): unknown keys, negative or non-integer counts and widths, more masks of a kind than the
    kernel draws, a ratio outside [0, 1], audio keys without an audio stream, video keys without a video stream, a freq_bins that
    does not divide the feature width (audio_feat, when given) or contradicts audio_processing='wav', an unknown mask_value."""
    if spec is None:
        return {}
    if not isinstance(spec, dict):
        raise ValueError("spec_augment must be None or a dict over %s (got %r)" % (", ".join(SPEC_AUGMENT_KEYS), type(spec).__name__))
    for k in spec:
        if k not in SPEC_AUGMENT_KEYS:
            raise ValueError("spec_augment: unknown key %r (the keys are %s)" % (k, ", ".join(SPEC_AUGMENT_KEYS)))
    out = {}
    for k in ("freq_masks", "freq_width", "time_masks", "time_width", "video_time_masks", "video_time_width"):
        v = spec.get(k, 0)
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise ValueError("spec_augment: %s must be a non-negative integer (got %r)" % (k, v))
        if k.endswith("masks") and v > SPEC_AUGMENT_MAX_MASKS:
            raise ValueError("spec_augment: %s: avsr_spec_augment draws at most %d masks of a kind (got %d)" % (k, SPEC_AUGMENT_MAX_MASKS, v))
        out["spec_" + k] = v
    for k in ("time_ratio", "video_time_ratio"):
        v = spec.get(k, 1.0)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 <= v <= 1.0:
            raise ValueError("spec_augment: %s must be a number in [0, 1] (got %r)" % (k, v))
        out["spec_" + k] = float(v)
    mv = spec.get("mask_value", "mean")
    if mv not in ("mean", "zero"):
        raise ValueError("spec_augment: mask_value must be 'mean' or 'zero' (got %r)" % (mv,))
    out["spec_mask_value"] = mv
    for k in spec:
        if k.startswith("video_") and not video:
            raise ValueError("spec_augment: %s needs a video stream (video_processing is None)" % k)
        if k in ("freq_masks", "freq_width", "freq_bins", "time_masks", "time_width", "time_ratio") and not audio:
            raise ValueError("spec_augment: %s needs an audio stream (audio_processing is None)" % k)
    fb = spec.get("freq_bins")
    if fb is not None:
        if isinstance(fb, bool) or not isinstance(fb, int) or fb < 1:
            raise ValueError("spec_augment: freq_bins must be a positive integer or None (got %r)" % (fb,))
        if audio_processing == "wav" and fb != num_mel_bins:
            raise ValueError("spec_augment: freq_bins is num_mel_bins (%d) with audio_processing='wav' (got %d)" % (num_mel_bins, fb))
        if audio_processing != "wav" and audio_feat is not None and audio_feat % fb:
            raise ValueError("spec_augment: freq_bins (%d) must divide the audio feature width (%d)" % (fb, audio_feat))
        out["spec_freq_bins"] = fb
    return out


def _video_augment_check(flip, max_shift, contrast, brightness, video_hw, name=lambda k: k):
    """The ranges of the four values; `name` turns a key into what the message calls it."""
    num = lambda v: not isinstance(v, bool) and isinstance(v, (int, float))
    if not num(flip) or not 0.0 <= flip <= 1.0:
        raise ValueError("%s must be a probability in [0, 1] (got %r)" % (name("flip"), flip))
    if isinstance(max_shift, bool) or not isinstance(max_shift, int) or not 0 <= max_shift < min(video_hw[0], video_hw[1]):
        raise ValueError("%s must be an integer with 0 <= max_shift < min(H, W) = %d (got %r)"
                         % (name("max_shift"), min(video_hw[0], video_hw[1]), max_shift))
    if not num(contrast) or not 0.0 <= contrast < 1.0:
        raise ValueError("%s must be a number in [0, 1) (got %r)" % (name("contrast"), contrast))
    if not num(brightness) or not 0.0 <= brightness < float("inf"):
        raise ValueError("%s must be a finite number >= 0 (got %r)" % (name("brightness"), brightness))


def video_augment_fields(spec, video_processing="resnet_cnn", video_hw=(36, 36, 3)):
    """The `video_augment` keyword of avsr.AVSR (None, or a dict over VIDEO_AUGMENT_KEYS) -> the ModelConfig fields it sets.  Refuses on
    the host, naming the key (ValueError): not a dict, unknown keys, a value outside its range (bools are no numbers), a video stream
    that holds no pixels (video_processing None or 'features')."""
    if spec is None:
        return {}
    if not isinstance(spec, dict):
        raise ValueError("video_augment must be None or a dict over %s (got %r)" % (", ".join(VIDEO_AUGMENT_KEYS), type(spec).__name__))
    for k in spec:
        if k not in VIDEO_AUGMENT_KEYS:
            raise ValueError("video_augment: unknown key %r (the keys are %s)" % (k, ", ".join(VIDEO_AUGMENT_KEYS)))
    if video_processing not in ("resnet_cnn", "3dconv_cnn"):
        raise ValueError("video_augment needs lip crops (video_processing='resnet_cnn' or '3dconv_cnn'; got %r): there are no pixels"
                         % (video_processing,))
    v = {k: spec.get(k, 0) for k in VIDEO_AUGMENT_KEYS}
    _video_augment_check(video_hw=video_hw, name=lambda k: "video_augment: " + k, **v)
    return dict(vaug_flip_q24=int(round(v["flip"] * 16777216.0)), vaug_max_shift=v["max_shift"], vaug_contrast=float(v["contrast"]),
                vaug_brightness=float(v["brightness"]))


def encoder_cell_id(stream, direction, layer):
    """RNG stream family of a DropoutWrapper'd encoder cell (stream = cell_id*4 + {0 input, 1 state, 2 output})."""
    return 1 + ((0 if stream == "video" else 1) * 2 + (0 if direction == "fw" else 1)) * 8 + layer


@dataclass
class ModelConfig:
    architecture: str = "unimodal"
    encoder_type: str = "unidirectional"
    cell_type: str = "lstm"
    video_units: Optional[Tuple[int, ...]] = None      # encoder_units_per_layer[0]; None = no video stream
    audio_units: Optional[Tuple[int, ...]] = (256, 256, 256)
    decoder_units: Tuple[int, ...] = (256,)
    attention_type: Tuple[Tuple[str, ...], Tuple[str, ...]] = (("scaled_luong",), ("scaled_luong",))
    enable_attention: bool = True
    embedding_size: int = 128
    vocab_size: int = 31
    go_id: int = 30
    eos_id: int = 29
    video_feat: int = 128
    audio_feat: int = 80
    batch_normalisation: bool = True
    regress_aus: bool = False
    au_loss_weight: float = 10.0
    # CTC auxiliary loss on the encoder outputs (not in the reference, whose hyper-parameter bag only reserves the switch): a Dense head
    # over vocab_size + 1 classes (the blank is the last) on the audio encoder if there is one, else the video encoder; its loss, per
    # label token like the sequence loss, is added with weight ctc_weight (0.3: a conventional value, not a tuned one)
    use_ctc: bool = False
    ctc_weight: float = 0.3
    recurrent_l2: Optional[float] = 1e-4
    clip_gradients: bool = True
    max_gradient_norm: float = 1.0
    learning_rate: float = 1e-3
    warmup_steps: int = 750
    optimiser: str = "Adam"                   # Adam | Nadam | AdamW | Momentum (seq2seq.py:195-218)
    weight_decay: float = 1e-4                # AdamW only (avsr.py:45)
    loss_fun: Optional[str] = None            # None | 'focal_loss' | 'mc_loss' (seq2seq.py:147-163, avsr/devel.py:12-51)
    label_smoothing: float = 0.0              # > 0: tf.losses.softmax_cross_entropy path (seq2seq.py:151-155)
    lr_decay_steps: int = 0                   # lr_decay=('cosine_restarts', N) (seq2seq.py:266-270); 0 = constant lr
    max_label_length: int = 150
    use_dropout: bool = False
    video_dropout: Tuple[float, float, float] = (0.9, 0.9, 0.9)     # keep probabilities (input, state, output), avsr.py:52-54
    audio_dropout: Tuple[float, float, float] = (0.9, 0.9, 0.9)
    decoder_dropout: Tuple[float, float, float] = (0.9, 0.9, 0.9)
    sampling_probability: float = 0.0
    # visual front-end (avsr/avsr.py:24, :33-34): "features" = records already hold cnn_dense_units-d vectors,
    # "resnet_cnn" = lip crops [B, T, H, W, C] through video.resnet_cnn (cnn.py), "3dconv_cnn" = through video.conv3d_cnn (cnn3d.py)
    video_processing: str = "features"
    # audio front-end (avsr/avsr.py:27): "features" = records already hold audio_feat-d vectors, "wav" = records hold samples and the
    # dataset writer's log-mel pipeline runs inside the model (audio_frontend.py); audio_feat is then num_mel_bins * stacking window
    audio_processing: str = "features"
    audio_transformation: str = "logmel_stack_w8s3"                 # | "logmel_stack_w3s3" | "logmel" (dataset_writer.py:357-380)
    num_mel_bins: int = 30                                          # dataset_writer.py:410
    sample_rate: int = 16000
    cnn_filters: Tuple[int, ...] = (8, 16, 32, 64)
    cnn_dense_units: int = 128
    video_hw: Tuple[int, int, int] = (36, 36, 3)
    input_dense_layers: Tuple[int, ...] = (0,)                      # avsr/avsr.py:38, encoder.py:148-171
    encoder_weight_sharing: bool = False                            # cells.py:77: encoder layers >= 2 reuse layer 1's cell
    instance_normalisation: bool = False                            # encoder.py:51-55: instance_norm after the batch norm
    highway_encoder: bool = False                                   # cells.py:89-90: HighwayWrapper on encoder layers > 0 (wins over residual)
    residual_encoder: bool = False                                  # cells.py:91-92: ResidualWrapper on encoder layers > 0
    # SpecAugment on the encoders' inputs in the train graph (not in the reference; csrc/specaugment.hip):
    # `*_masks` bands / spans of up to `*_width` bins / rows, a span also of at most `*_ratio` of the utterance; every count defaults to
    # 0 = off, and no size here is tuned.  spec_freq_bins: period of the frequency axis (0 = num_mel_bins with audio_processing='wav',
    # else the feature width).  spec_augment_fields() turns avsr.AVSR's `spec_augment` dict into these.
    spec_freq_masks: int = 0
    spec_freq_width: int = 0
    spec_freq_bins: int = 0
    spec_time_masks: int = 0
    spec_time_width: int = 0
    spec_time_ratio: float = 1.0
    spec_video_time_masks: int = 0
    spec_video_time_width: int = 0
    spec_video_time_ratio: float = 1.0
    spec_mask_value: str = "mean"                                   # 'mean' (the utterance's own column mean) | 'zero'
    # Lip-crop augmentation in the train graph (not in the reference, which lists the intent at the top of its resnet_cnn();
    # csrc/video_augment.hip), per utterance: a horizontal flip with probability vaug_flip_q24 / 2^24, a shift of
    # up to vaug_max_shift pixels per axis, a contrast factor 1 +- vaug_contrast, a brightness offset +- vaug_brightness.  Every value
    # defaults to 0 = off, and none is tuned.  video_augment_fields() turns avsr.AVSR's `video_augment` dict into these.
    vaug_flip_q24: int = 0
    vaug_max_shift: int = 0
    vaug_contrast: float = 0.0
    vaug_brightness: float = 0.0
    one_hot_embedding: bool = False      # set by engine(): embedding_size <= 0 -> tf.eye(vocab_size) decoder inputs (decoder_unimodal.py:76-77)

    # -- same helpers/validation rules as the reference wiring (error types as in the reference) --
    def streams(self) -> List[str]:
        s = []
        if self.video_units is not None:
            s.append("video")
        if self.audio_units is not None:
            s.append("audio")
        return s

    def wrapped(self, stream: str) -> bool:
        """Do residual_encoder / highway_encoder / encoder_weight_sharing reach this stream's stack?  Only the unidirectional
        branch of Seq2SeqEncoder hands them to build_rnn_layers (encoder.py:67-78); the bidirectional branch builds _fw_cells /
        _bw_cells without them (encoder.py:92-108) and so does AttentiveEncoder for the AV-Align audio stack (encoder.py:225-233):
        there the reference silently ignores the flags, and so does this engine."""
        return self.encoder_type == "unidirectional" and not (self.architecture == "av_align" and stream == "audio")

    def highway(self, stream: str) -> bool:
        return self.highway_encoder and self.wrapped(stream)

    def residual(self, stream: str) -> bool:
        return self.residual_encoder and not self.highway_encoder and self.wrapped(stream)      # cells.py:89-92: highway wins

    def shared_layer(self, stream: str, l: int) -> int:
        """Index of the encoder layer whose variables layer l uses (cells.py:77 quirk: `layer > 1` reuses cell_list[-1], so
        layers 0 and 1 stay distinct and every layer from 2 up is layer 1's cell)."""
        return 1 if (self.encoder_weight_sharing and self.wrapped(stream) and l > 1) else l

    def loss_code(self) -> int:
        """avsr_seq_loss_fun's loss_fun argument."""
        if self.loss_fun is None:
            return 1 if self.label_smoothing > 0.0 else 0
        if self.loss_fun not in ("focal_loss", "mc_loss"):
            raise ValueError('Unknown loss function {}'.format(self.loss_fun))          # seq2seq.py:163
        return 2 if self.loss_fun == "focal_loss" else 3

    def directions(self) -> List[str]:
        return ["fw", "bw"] if self.encoder_type == "bidirectional" else ["fw"]

    def ctc_stream(self) -> Optional[str]:
        """The stream whose encoder carries the CTC head; None when use_ctc is off."""
        if not self.use_ctc:
            return None
        return "audio" if self.audio_units is not None else "video"

    def units(self, stream):
        return self.video_units if stream == "video" else self.audio_units

    def spec_augment_args(self, stream: str) -> Optional[dict]:
        """The draw parameters of avsr_spec_augment for this stream's input in the train graph; None = nothing to launch (the
        switch is off, or every mask of the stream is empty by construction)."""
        if stream not in self.streams():
            return None
        q16 = lambda r: int(round(r * 65536.0))
        if stream == "video":
            a = dict(video=True, time_masks=self.spec_video_time_masks, time_width=self.spec_video_time_width,
                     ratio_q16=q16(self.spec_video_time_ratio))
        else:
            a = dict(video=False, time_masks=self.spec_time_masks, time_width=self.spec_time_width, ratio_q16=q16(self.spec_time_ratio),
                     freq_masks=self.spec_freq_masks, freq_width=self.spec_freq_width, freq_bins=self.spec_freq_bins)
            if not (a["freq_masks"] > 0 and a["freq_width"] > 0):
                a.update(freq_masks=0, freq_width=0, freq_bins=0)
        if not (a["time_masks"] > 0 and a["time_width"] > 0 and a["ratio_q16"] > 0):
            a.update(time_masks=0, time_width=0)
        if not a["time_masks"] and not a.get("freq_masks"):
            return None
        a["mean_fill"] = self.spec_mask_value == "mean"
        return a

    def video_augment_args(self) -> Optional[dict]:
        """The parameters of avsr_video_augment for the lip crops in the train graph; None = nothing to launch (every value is 0, or
        the video stream holds no pixels)."""
        if self.video_units is None or self.video_processing not in ("resnet_cnn", "3dconv_cnn"):
            return None
        a = dict(flip_q24=self.vaug_flip_q24, max_shift=self.vaug_max_shift, contrast=self.vaug_contrast, brightness=self.vaug_brightness)
        return a if any(a.values()) else None

    def one_hot(self) -> bool:
        """decoder_unimodal.py:76-77: a non-positive embedding_size falls back to one-hot decoder inputs (no embedding variable)."""
        return self.one_hot_embedding or self.embedding_size <= 0

    def emb_width(self) -> int:
        return self.embedding_size if self.embedding_size > 0 else self.vocab_size

    def engine(self) -> "ModelConfig":
        """The configuration the kernels run: every feature / unit / embedding width rounded up to a multiple of 4 (16-byte rows,
        whole MFMA unit groups).  Padding entries of every variable are zero and stay zero (a padded LSTM / GRU unit has zero
        weights and bias: its candidate is tanh(0) = 0, so its cell and output stay 0; every consumer's rows for it are zero, so
        it receives a zero gradient and so do its weights) - the padded model computes exactly the unpadded one.
        `params.embed` / `params.extract` convert between the two layouts; the reference's shapes are what is imported / exported."""
        r = lambda t: None if t is None else tuple(round4(u) for u in t)
        dense = self.input_dense_layers if self.input_dense_layers[0] <= 0 else tuple(round4(u) for u in self.input_dense_layers)
        # (the period of the SpecAugment bands is settled on the reference's width, before it is padded)
        bins = self.spec_freq_bins
        if self.spec_freq_masks and not bins:
            bins = self.num_mel_bins if self.audio_processing == "wav" else self.audio_feat
        return replace(self, video_units=r(self.video_units), audio_units=r(self.audio_units), decoder_units=r(self.decoder_units),
                       embedding_size=round4(self.emb_width()), video_feat=round4(self.video_feat), audio_feat=round4(self.audio_feat),
                       input_dense_layers=dense, one_hot_embedding=self.one_hot(), spec_freq_bins=bins)

    def feat(self, stream):
        return self.video_feat if stream == "video" else self.audio_feat

    def layer0_in(self, stream: str) -> int:
        """Width of the first encoder layer's input: the last input Dense layer if any, else the feature size."""
        return self.input_dense_layers[-1] if self.input_dense_layers[0] > 0 else self.feat(stream)

    def memory_depth(self, stream: str) -> int:
        return self.units(stream)[-1] * (2 if self.encoder_type == "bidirectional" else 1)

    def decoder_memories(self) -> List[Tuple[str, str]]:
        """[(stream, attention_type)] in AttentionWrapper order (decoder_bimodal.py:184-223: video first)."""
        if not self.enable_attention or self.architecture == "lm":
            return []
        if self.architecture == "bimodal":
            out = []
            if self.video_units is not None:
                out += [("video", t) for t in self.attention_type[0]]
            if self.audio_units is not None:
                out += [("audio", t) for t in self.attention_type[1]]
            return out
        stream = "audio" if self.audio_units is not None else "video"
        return [(stream, t) for t in self.attention_type[1]]

    def output_attention(self) -> bool:
        mems = self.decoder_memories()
        return bool(mems) and mems[-1][1] in LUONG_TYPES

    def _validate_spec_augment(self):
        counts = ("spec_freq_masks", "spec_freq_width", "spec_time_masks", "spec_time_width", "spec_video_time_masks",
                  "spec_video_time_width", "spec_freq_bins")
        for k in counts:
            v = getattr(self, k)
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise ValueError("%s must be a non-negative integer (got %r)" % (k, v))
            if k.endswith("masks") and v > SPEC_AUGMENT_MAX_MASKS:
                raise ValueError("%s: avsr_spec_augment draws at most %d masks of a kind (got %d)" % (k, SPEC_AUGMENT_MAX_MASKS, v))
        for k in ("spec_time_ratio", "spec_video_time_ratio"):
            if not 0.0 <= getattr(self, k) <= 1.0:
                raise ValueError("%s must lie in [0, 1] (got %r)" % (k, getattr(self, k)))
        if self.spec_mask_value not in ("mean", "zero"):
            raise ValueError("spec_mask_value must be 'mean' or 'zero' (got %r)" % (self.spec_mask_value,))
        if (self.spec_freq_masks or self.spec_time_masks) and self.audio_units is None:
            raise ValueError("spec_freq_masks / spec_time_masks need an audio stream")
        if self.spec_video_time_masks and self.video_units is None:
            raise ValueError("spec_video_time_masks needs a video stream")
        if self.spec_freq_bins and self.audio_units is not None:
            P = self.spec_freq_bins
            if self.audio_processing == "wav":
                if P != self.num_mel_bins:
                    raise ValueError("spec_freq_bins is num_mel_bins (%d) with audio_processing='wav' (got %d)" % (self.num_mel_bins, P))
            # (audio_feat may already be the engine's 4-padded width, as for the waveform front-end's check below: the period
            # must divide a width that pads to it)
            elif not any(w % P == 0 for w in range(self.audio_feat, self.audio_feat - 4, -1)
                         if w >= 1 and (w == self.audio_feat or (self.audio_feat % 4 == 0 and round4(w) == self.audio_feat))):
                raise ValueError("spec_freq_bins (%d) must divide the audio feature width (%d)" % (P, self.audio_feat))

    def _validate_video_augment(self):
        q = self.vaug_flip_q24
        if isinstance(q, bool) or not isinstance(q, int) or not 0 <= q <= 1 << 24:
            raise ValueError("vaug_flip_q24 must be an integer in [0, 2^24] (got %r)" % (q,))
        _video_augment_check(0.0, self.vaug_max_shift, self.vaug_contrast, self.vaug_brightness, self.video_hw, name=lambda k: "vaug_" + k)
        if q or self.vaug_max_shift or self.vaug_contrast or self.vaug_brightness:
            if self.video_units is None or self.video_processing not in ("resnet_cnn", "3dconv_cnn"):
                raise ValueError("vaug_* need lip crops (a video stream with video_processing='resnet_cnn' or '3dconv_cnn'): "
                                 "there are no pixels")

    def validate(self):
        if self.architecture == "lm":                                                 # avsr.LM (lm.py:275-471): labels only, no encoders
            if self.video_units is not None or self.audio_units is not None:
                raise ValueError("the language model has no encoders")
        elif self.architecture not in ("unimodal", "bimodal", "av_align"):
            raise Exception("Unknown architecture")                                   # seq2seq.py:66
        if self.encoder_type not in ("unidirectional", "bidirectional"):
            raise Exception("Allowed encoder types: `unidirectional`, `bidirectional`")  # encoder.py:146
        if self.cell_type not in ("lstm", "gru"):
            raise Exception("cell type not supported: {}".format(self.cell_type))      # cells.py:44
        for types in self.attention_type:
            for t in types:
                if t not in ATT_CODE:
                    raise Exception("unknown attention mechanism")                    # attention.py:86
        if self.architecture == "bimodal" and self.cell_type != "lstm":
            raise ValueError("the bimodal decoder needs LSTM state tuples (decoder_bimodal.py:130-142, :484-485)")
        if self.architecture == "av_align":
            if self.encoder_type != "unidirectional":
                raise ValueError("AttentiveEncoder implements only `unidirectional` (encoder.py:229)")
            if self.video_units is None or self.audio_units is None:
                raise ValueError("av_align needs both a video and an audio stream")
        self.loss_code()
        if self.use_ctc:
            if self.architecture == "lm":
                raise ValueError("use_ctc: the language model has no encoder to put the CTC head on")
            if self.label_smoothing > 0.0:
                raise ValueError("use_ctc with label_smoothing > 0: the sequence loss is then normalised by label rows, not label "
                                 "tokens, and the CTC term shares its normaliser")
            if self.ctc_weight < 0.0:
                raise ValueError("ctc_weight must not be negative")
            if not self.enable_attention:
                raise NotImplementedError("use_ctc with enable_attention=False is not built")
        self._validate_spec_augment()
        self._validate_video_augment()
        if self.optimiser not in ("Adam", "Nadam", "AdamW", "Momentum"):
            raise Exception('Unsupported optimiser, try Adam')                            # seq2seq.py:218
        for st in self.streams():                 # the wrapper flags only where the reference applies them (see `wrapped`)
            u = self.units(st)
            if self.highway(st) and self.encoder_weight_sharing:
                raise NotImplementedError("highway_encoder with encoder_weight_sharing")
            if self.highway(st) or self.residual(st):
                if len(set(u)) != 1:
                    raise ValueError("residual_encoder needs equal layer widths")
            if self.encoder_weight_sharing and self.wrapped(st):
                if len(u) > 2 and (len(set(u[1:])) != 1 or u[0] != u[1]):
                    raise ValueError("encoder_weight_sharing needs equal layer sizes: layers >= 2 reuse layer 1's kernel")
        if self.video_processing not in ("features", "resnet_cnn", "3dconv_cnn"):
            raise Exception("unknown visual content")                                   # avsr/avsr.py:713 (2dconv_cnn: not built)
        if self.video_units is not None and self.video_processing == "3dconv_cnn":
            c = self.video_hw[2]
            if max(self.cnn_filters) > 128 or c > 128 or (c > 3 and c % 4):
                raise ValueError("3dconv_cnn: cnn_filters up to 128, frames of 1-3 or 4n <= 128 channels (avsr_conv3d_supported)")
        if self.video_units is not None and self.video_processing in ("resnet_cnn", "3dconv_cnn"):
            if self.video_feat != self.cnn_dense_units:
                raise ValueError("video_feat must equal cnn_dense_units when the CNN front-end produces the video features")
            if any(c % 4 for c in self.cnn_filters) or self.cnn_dense_units % 4 or len(self.cnn_filters) < 1:
                raise ValueError("cnn_filters / cnn_dense_units must be multiples of 4 for the HIP engine")
        if self.audio_processing not in ("features", "wav"):
            raise NotImplementedError("audio_processing=%r: 'features' and 'wav' are built" % (self.audio_processing,))
        if self.audio_units is not None and self.audio_processing == "wav":
            from .audio_frontend import spec_from_config
            spec = spec_from_config(self)                  # raises for the refused transformations / sample rates / filter counts
            if self.audio_feat not in (spec.feat, round4(spec.feat)):
                raise ValueError("audio_feat must equal num_mel_bins * stacking window (%d) when the waveform front-end produces the "
                                 "audio features" % spec.feat)
        if self.input_dense_layers[0] > 0 and any(u <= 0 for u in self.input_dense_layers):
            raise ValueError("input_dense_layers must be positive")
        if len(set(self.decoder_units)) != 1 or len(self.decoder_units) > 4:
            raise NotImplementedError("multi-layer decoders: up to 4 layers of equal width")
        if not self.streams() and self.architecture != "lm":
            raise Exception("labels are None")                                         # seq2seq.py:94
        dims = [self.decoder_units[0]]
        for s in self.streams():
            dims += list(self.units(s)) + [self.feat(s)]
        if any(d <= 0 for d in dims):
            raise ValueError("feature / unit sizes must be positive")       # other widths: padded inside the engine (`engine()`)
