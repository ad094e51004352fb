"""ctypes binding of libavsr_hip.so (C ABI declared in include/avsr_hip.h).

The product path has NO CPU fallback: if the shared library is missing or an entry point fails,
an exception is raised.  torch must be imported before the library is loaded so that the HIP
runtime (libamdhip64.so.7) already mapped by torch is the one our kernels launch on.
"""
import ctypes as C
import os

import torch  # noqa: F401  (must precede CDLL: shares torch's HIP runtime instance)

from . import build as _build

MAX_LAYERS = 4
MAX_MECH = 4
MAX_STACKS = 4

_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)


class AvsrError(RuntimeError):
    pass


class Mat(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("ld", C.c_int64), ("T", C.c_int32), ("pad_", C.c_int32), ("ldo", C.c_int64)]


class GemmDesc(C.Structure):
    _fields_ = [("A", Mat), ("B", Mat), ("C", Mat), ("bias", C.c_void_p),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("trans_a", C.c_int32), ("trans_b", C.c_int32),
                ("alpha", C.c_float), ("beta", C.c_float), ("batch", C.c_int32),
                ("stride_a", C.c_int64), ("stride_b", C.c_int64), ("stride_c", C.c_int64),
                ("alpha_dev", C.c_void_p),
                ("splitk", C.c_int32), ("pad_", C.c_int32),
                ("workspace", C.c_void_p), ("workspace_floats", C.c_int64),
                ("colsum", C.c_void_p), ("colsum_beta", C.c_float), ("pad2_", C.c_int32)]


class RnnLayer(C.Structure):
    _fields_ = [("units", C.c_int32), ("in_dim", C.c_int32), ("hoisted", C.c_int32), ("out_col", C.c_int32),
                ("wt", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p),
                ("gates", C.c_void_p), ("cs", C.c_void_p), ("out", C.c_void_p), ("ld_out", C.c_int64),
                ("state", C.c_void_p), ("h_final", C.c_void_p), ("c_final", C.c_void_p),
                ("dgates", C.c_void_p), ("dstate", C.c_void_p), ("dout", C.c_void_p), ("ld_dout", C.c_int64),
                ("dout_col", C.c_int32), ("residual", C.c_int32), ("hs_seq", C.c_void_p), ("xt_seq", C.c_void_p),
                ("wt2", C.c_void_p), ("w2", C.c_void_p), ("bias2", C.c_void_p), ("rh_seq", C.c_void_p), ("dgates2", C.c_void_p)]


class RnnStack(C.Structure):
    _fields_ = [("B", C.c_int32), ("T", C.c_int32), ("reverse", C.c_int32), ("n_layers", C.c_int32),
                ("cell", C.c_int32), ("pad_", C.c_int32),
                ("len", C.c_void_p), ("dh_final", C.c_void_p), ("dc_final", C.c_void_p),
                ("seed", C.c_void_p), ("keep_in", C.c_float), ("keep_state", C.c_float), ("keep_out", C.c_float),
                ("consumer_keep", C.c_float), ("cell_id_base", C.c_int32), ("consumer_stream", C.c_int32),
                ("consumer_width", C.c_int32), ("pad2_", C.c_int32),
                ("layer", RnnLayer * MAX_LAYERS)]


class RnnLaunch(C.Structure):
    """avsr_rnn_launch: one record of avsr_rnn_plan."""
    _fields_ = [(n, C.c_int32) for n in ("form", "stacks", "rows_per_group", "rows_per_slice", "launches", "wg_per_xcd", "crossing_edges",
                                         "top_tiles")]


class AttnMech(C.Structure):
    _fields_ = [("type", C.c_int32), ("T", C.c_int32), ("D", C.c_int32), ("chunk", C.c_int32),
                ("len", C.c_void_p), ("keys", C.c_void_p), ("values", C.c_void_p),
                ("values_sb", C.c_int64), ("values_st", C.c_int64),
                ("g", C.c_void_p), ("v", C.c_void_p), ("bq", C.c_void_p),
                ("wq_t", C.c_void_p), ("wq", C.c_void_p), ("watt_t", C.c_void_p), ("watt", C.c_void_p),
                ("scores", C.c_void_p), ("ctx", C.c_void_p), ("pq", C.c_void_p), ("pstat", C.c_void_p),
                ("pctx", C.c_void_p), ("dscores", C.c_void_p), ("dctx", C.c_void_p), ("dpq", C.c_void_p),
                ("pdq", C.c_void_p)]


class DecLayer(C.Structure):
    _fields_ = [("wt", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("gates", C.c_void_p), ("cs", C.c_void_p),
                ("out", C.c_void_p), ("state", C.c_void_p), ("hs_seq", C.c_void_p), ("xin_seq", C.c_void_p),
                ("dgates", C.c_void_p), ("dstate", C.c_void_p), ("cell_id", C.c_int32), ("pad_", C.c_int32),
                ("wt2", C.c_void_p), ("w2", C.c_void_p), ("bias2", C.c_void_p), ("rh_seq", C.c_void_p), ("dgates2", C.c_void_p)]


MAX_DEC_EXTRA = 3


class AttnRnn(C.Structure):
    _fields_ = [("B", C.c_int32), ("L", C.c_int32), ("H", C.c_int32), ("E", C.c_int32),
                ("n_mech", C.c_int32), ("output_attention", C.c_int32), ("V", C.c_int32), ("mode", C.c_int32),
                ("go_id", C.c_int32), ("eos_id", C.c_int32),
                ("steplen", C.c_void_p), ("wt", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p),
                ("gates", C.c_void_p), ("cs", C.c_void_p), ("cell_out", C.c_void_p), ("att", C.c_void_p),
                ("h0", C.c_void_p), ("c0", C.c_void_p), ("state", C.c_void_p),
                ("h_final", C.c_void_p), ("c_final", C.c_void_p),
                ("mech", AttnMech * MAX_MECH),
                ("embedding", C.c_void_p), ("wout_t", C.c_void_p), ("bout", C.c_void_p),
                ("logits", C.c_void_p), ("ids", C.c_void_p), ("tok", C.c_void_p), ("n_unfinished", C.c_void_p),
                ("dgates", C.c_void_p), ("dstate", C.c_void_p), ("datt", C.c_void_p), ("dq", C.c_void_p),
                ("datt_ext", C.c_void_p), ("dcell_ext", C.c_void_p), ("dh0", C.c_void_p), ("dc0", C.c_void_p),
                ("dh_final", C.c_void_p), ("dc_final", C.c_void_p),
                ("seed", C.c_void_p), ("keep_in", C.c_float), ("keep_state", C.c_float), ("keep_out", C.c_float),
                ("sampling_prob", C.c_float), ("cell_id", C.c_int32), ("pad3_", C.c_int32),
                ("hs_seq", C.c_void_p), ("attd", C.c_void_p), ("xs", C.c_void_p), ("labels", C.c_void_p), ("fed", C.c_void_p),
                ("cell", C.c_int32), ("pad4_", C.c_int32), ("wt2", C.c_void_p), ("w2", C.c_void_p), ("bias2", C.c_void_p),
                ("rh_seq", C.c_void_p), ("dgates2", C.c_void_p),
                ("beam_width", C.c_int32), ("mem_shared", C.c_int32), ("length_penalty", C.c_float), ("pad6_", C.c_float),
                ("beam_logp", C.c_void_p), ("beam_fin", C.c_void_p), ("beam_len", C.c_void_p), ("step_ids", C.c_void_p),
                ("parent_ids", C.c_void_p), ("parent_rows", C.c_void_p),
                ("n_extra", C.c_int32), ("prof_tag", C.c_int32), ("out0", C.c_void_p), ("extra", DecLayer * MAX_DEC_EXTRA),
                ("fused_ws", C.c_void_p), ("fused_ws_floats", C.c_int64)]


class AttnRnnLaunch(C.Structure):
    """avsr_attn_rnn_launch: the record of avsr_attn_rnn_plan."""
    _fields_ = [(n, C.c_int32) for n in ("form", "variant", "rows_per_group", "v64", "launches", "pad_")] + \
               [("quarter", C.c_int32 * MAX_MECH), ("lds_bytes", C.c_int64)]


MAX_LM_LAYERS = 4


class BeamLm(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("H", C.c_int32), ("E", C.c_int32), ("V", C.c_int32),
                ("one_hot", C.c_int32), ("n_rows", C.c_int32), ("lm_weight", C.c_float), ("pad_", C.c_int32),
                ("embedding", C.c_void_p), ("wt", C.c_void_p * MAX_LM_LAYERS), ("bias", C.c_void_p * MAX_LM_LAYERS),
                ("wout_t", C.c_void_p), ("bout", C.c_void_p), ("state_c", C.c_void_p), ("state_h", C.c_void_p), ("lm_logp", C.c_void_p)]


BEAM_CTC_MAX_T, BEAM_CTC_MAX_V = 2048, 256          # AVSR_BEAM_CTC_MAX_T / _V of include/avsr_hip.h


class BeamCtc(C.Structure):
    _fields_ = [("n_utt", C.c_int32), ("beam_width", C.c_int32), ("T", C.c_int32), ("V", C.c_int32), ("eos_id", C.c_int32),
                ("weight", C.c_float), ("ld", C.c_int64)] + \
               [(n, C.c_void_p) for n in ("z", "in_len", "y", "state", "psi", "last", "term", "extra", "lm_logp")] + \
               [("lm_weight", C.c_float), ("pad_", C.c_int32)]


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("N", "H", "W", "Ci", "Co", "k", "stride", "pad_t", "pad_l", "Ho", "Wo", "pad_")] + \
               [("bn_scale", C.c_void_p), ("bn_shift", C.c_void_p)]


class ConvLaunch(C.Structure):
    """avsr_conv_launch: one record of avsr_conv_plan."""
    _fields_ = [(n, C.c_int32) for n in ("kernel", "m", "ntc", "ch4", "rs", "fold", "ep", "nsp", "ntap", "t0", "F", "grid", "CsP", "lds_bytes",
                                         "slab", "pad_")]


class BnPlan(C.Structure):
    """avsr_bn_plan: the launch geometry avsr_batchnorm_plan reports."""
    _fields_ = [(n, C.c_int32) for n in ("blocks", "rows_per_block", "G", "vec", "direct", "apply_grid", "err", "pad_")]


class Conv3dDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "T", "H", "W", "Ci", "Co", "kt", "kh", "kw", "stride", "pad_f", "pad_t", "pad_l", "Ho", "Wo",
                                         "relu")] + [("scale", C.c_void_p), ("shift", C.c_void_p)]


class LogmelArgs(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "N", "T_out", "F", "frame_length", "frame_step", "fft_length", "num_mel_bins", "window", "stride",
                                         "mel_nnz", "pad_")] + \
               [(n, C.c_void_p) for n in ("wav", "wav_len", "hann", "twiddle", "mel_lo", "mel_cnt", "mel_ptr", "mel_w", "out", "out_len")]


SPEC_AUGMENT_MAX_MASKS, SPEC_AUGMENT_MAX_T = 8, 65535          # AVSR_SPEC_AUGMENT_MAX_* of include/avsr_hip.h


class SpecAugmentArgs(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "T", "F_in", "F", "freq_masks", "freq_width", "freq_bins", "time_masks", "time_width",
                                         "ratio_q16", "video", "mean_fill")] + [("ld", C.c_int64)] + \
               [(n, C.c_void_p) for n in ("x", "len", "seed", "y", "ws")] + [("ws_floats", C.c_int64)]


VIDEO_AUGMENT_MAX_T, VIDEO_AUGMENT_MAX_C = 65535, 64            # AVSR_VIDEO_AUGMENT_MAX_* of include/avsr_hip.h


class VideoAugmentArgs(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "T", "H", "W", "C", "max_shift", "flip_q24", "pad_")] + \
               [("contrast", C.c_float), ("brightness", C.c_float)] + \
               [(n, C.c_void_p) for n in ("x", "len", "seed", "y", "ws")] + [("ws_floats", C.c_int64)]


class CtcArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("T", C.c_int32), ("L", C.c_int32), ("C", C.c_int32), ("ld", C.c_int64)] + \
               [(n, C.c_void_p) for n in ("z", "labels", "labels_len", "in_len", "denom")] + [("weight", C.c_float), ("pad_", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("nll", "status", "utt_loss", "dz", "ws")] + [("ws_floats", C.c_int64)]


CTC_PREFIX_MAX_V, CTC_PREFIX_MAX_W, CTC_PREFIX_MAX_L = 256, 64, 512     # AVSR_CTC_PREFIX_MAX_* of include/avsr_hip.h


class CtcPrefixArgs(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "T", "V", "beam_width", "L_max", "pad_")] + [("ld", C.c_int64)] + \
               [(n, C.c_void_p) for n in ("z", "in_len", "ids", "lens", "score", "trace_parent", "trace_sym", "trace_pb", "trace_pnb")]


CTC_PREFIX_LM_MAX_W = 16               # AVSR_CTC_PREFIX_LM_MAX_W of include/avsr_hip.h


class CtcPrefixLm(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_layers", "H", "E", "V", "one_hot", "go_id", "eos_id")] + \
               [("weight", C.c_float), ("bonus", C.c_float), ("pad_", C.c_int32), ("embedding", C.c_void_p),
                ("wt", C.c_void_p * MAX_LM_LAYERS), ("bias", C.c_void_p * MAX_LM_LAYERS), ("wout_t", C.c_void_p), ("bout", C.c_void_p),
                ("ws", C.c_void_p), ("ws_bytes", C.c_int64), ("s_lm", C.c_void_p), ("lm_steps", C.c_void_p), ("lm_logp", C.c_void_p)]


CTC_PREFIX_NGRAM_MAX_ORDER = 16        # AVSR_CTC_PREFIX_NGRAM_MAX_ORDER, _MAX_NODES, _MAX_ARCS of include/avsr_hip.h
CTC_PREFIX_NGRAM_MAX_NODES = 1 << 24
CTC_PREFIX_NGRAM_MAX_ARCS = 1 << 26


class CtcPrefixNgram(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_nodes", "n_arcs", "V", "start", "go_id", "eos_id")] + \
               [("weight", C.c_float), ("bonus", C.c_float)] + \
               [(n, C.c_void_p) for n in ("bow", "backoff", "arc_begin", "sym", "logp", "next", "s_lm", "lm_steps", "lm_logp")]


class CtcPrefixWordNgram(C.Structure):
    """avsr_ctc_prefix_word_ngram: a word automaton (CtcPrefixNgram's six tables over word ids) and the lexicon trie over its spellings
    (csrc/ctc_prefix_word_ngram.hip)."""
    _fields_ = [(n, C.c_int32) for n in ("n_nodes", "n_arcs", "Vw", "start", "eos_w", "unk_id", "n_trie_nodes", "n_trie_arcs", "V",
                                         "space_id", "go_id", "eos_id")] + \
               [("weight", C.c_float), ("bonus", C.c_float), ("oov", C.c_float), ("pad_", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("bow", "backoff", "arc_begin", "sym", "logp", "next", "t_begin", "t_sym", "t_next", "t_word",
                                          "s_lm", "lm_steps", "lm_logp")]


class BeamNgram(C.Structure):
    """avsr_beam_ngram: the automaton of CtcPrefixNgram as beam search's fused model (csrc/beam_ngram.hip)."""
    _fields_ = [(n, C.c_int32) for n in ("n_nodes", "n_arcs", "V", "start", "n_rows")] + [("lm_weight", C.c_float)] + \
               [(n, C.c_void_p) for n in ("bow", "backoff", "arc_begin", "sym", "logp", "next", "node", "lm_logp")]


class BeamWordNgram(C.Structure):
    """avsr_beam_word_ngram: the word automaton and lexicon trie of CtcPrefixWordNgram as beam search's fused model
    (csrc/beam_word_ngram.hip)."""
    _fields_ = [(n, C.c_int32) for n in ("n_nodes", "n_arcs", "Vw", "start", "eos_w", "unk_id", "n_trie_nodes", "n_trie_arcs", "V", "space_id",
                                         "go_id", "eos_id", "n_rows")] + \
               [("lm_weight", C.c_float), ("oov", C.c_float), ("pad_", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("bow", "backoff", "arc_begin", "sym", "logp", "next", "t_begin", "t_sym", "t_next", "t_word", "state",
                                          "lm_logp")]


CTC_ALIGN_MAX_L = 512                  # AVSR_CTC_ALIGN_MAX_L of include/avsr_hip.h


class CtcAlignArgs(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "T", "L", "V")] + [("ld", C.c_int64)] + \
               [(n, C.c_void_p) for n in ("z", "labels", "target_len", "in_len", "score", "status", "path", "frame_lp", "start", "end", "ws")] + \
               [("ws_bytes", C.c_int64)]


class ColsumJob(C.Structure):
    _fields_ = [("a", Mat), ("b", Mat), ("out", C.c_void_p), ("rows", C.c_int32), ("F", C.c_int32), ("alpha", C.c_float), ("beta", C.c_float)]


class TransposeJob(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("rows", C.c_int32), ("cols", C.c_int32)]


_STRUCTS = {"avsr_dec_layer": DecLayer, "avsr_mat": Mat, "avsr_gemm_desc": GemmDesc, "avsr_rnn_layer": RnnLayer, "avsr_rnn_stack": RnnStack,
            "avsr_rnn_launch": RnnLaunch,
            "avsr_conv_desc": ConvDesc, "avsr_conv_launch": ConvLaunch, "avsr_bn_plan": BnPlan, "avsr_conv3d_desc": Conv3dDesc, "avsr_logmel_args": LogmelArgs, "avsr_spec_augment_args": SpecAugmentArgs, "avsr_video_augment_args": VideoAugmentArgs, "avsr_ctc_args": CtcArgs, "avsr_attn_mech": AttnMech, "avsr_attn_rnn": AttnRnn, "avsr_transpose_job": TransposeJob,
            "avsr_attn_rnn_launch": AttnRnnLaunch,
            "avsr_colsum_job": ColsumJob, "avsr_beam_lm": BeamLm, "avsr_beam_ctc": BeamCtc, "avsr_ctc_prefix_args": CtcPrefixArgs,
            "avsr_ctc_prefix_lm": CtcPrefixLm, "avsr_ctc_prefix_ngram": CtcPrefixNgram, "avsr_ctc_prefix_word_ngram": CtcPrefixWordNgram,
            "avsr_beam_ngram": BeamNgram, "avsr_beam_word_ngram": BeamWordNgram,
            "avsr_ctc_align_args": CtcAlignArgs}

_vp, _i32, _i64, _f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
# argument types of every entry point that returns an int status (include/avsr_hip.h)
_SIGS = {
    "avsr_gemm": [C.POINTER(GemmDesc), _vp],
    "avsr_gemm_batch": [C.POINTER(GemmDesc), _i32, _vp],
    "avsr_rnn_fwd": [C.POINTER(RnnStack), _i32, _vp],
    "avsr_rnn_bwd": [C.POINTER(RnnStack), _i32, _vp],
    "avsr_rnn_set_persistent": [_vp, _i64],
    "avsr_rnn_set_persistent_mode": [_i32],
    "avsr_rnn_set_persistent_scratch": [_vp, _i64],
    "avsr_rnn_plan": [C.POINTER(RnnStack), _i32, _i32, _i32, _i64, _i64, C.POINTER(RnnLaunch), _i32],
    "avsr_attn_rnn_fwd": [C.POINTER(AttnRnn), _i32, _i32, _vp],
    "avsr_attn_rnn_fused_eligible": [C.POINTER(AttnRnn)],
    "avsr_attn_rnn_fused_fwd_active": [C.POINTER(AttnRnn)],
    "avsr_attn_rnn_set_fused": [_i32],
    "avsr_attn_rnn_plan": [C.POINTER(AttnRnn), _i32, C.POINTER(AttnRnnLaunch)],
    "avsr_attn_rnn_set_beam_kernel": [_i32],
    "avsr_conv_set_mfma": [_i32],
    "avsr_conv_supported": [C.POINTER(ConvDesc)],
    "avsr_conv_fwd": [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i32), _vp],
    "avsr_conv_bwd_data": [C.POINTER(ConvDesc), _vp, _vp, _vp, _f32, _vp],
    "avsr_conv_bwd_weight": [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _f32, _vp, _i64, _vp],
    "avsr_conv_bwd_data_bn": [C.POINTER(ConvDesc), _vp, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i32), _vp],
    "avsr_conv_bwd_data_bn_supported": [C.POINTER(ConvDesc)],
    "avsr_conv_bwd_weight_bn": [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _i64, _vp],
    "avsr_conv_bwd_weight_bn_supported": [C.POINTER(ConvDesc)],
    "avsr_conv_plan": [C.POINTER(ConvDesc), _i32, _i32, _i64, C.POINTER(ConvLaunch), _i32],
    "avsr_batchnorm_plan": [_i32, _i64, _i32, _i64, _i32, C.POINTER(BnPlan)],
    "avsr_bn_bwd_finalize": [_vp, _i32, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _vp],
    "avsr_bn_bwd_apply": [_vp, _vp, _vp, _vp, _i64, _i32, _f32, _vp],
    "avsr_bn_bwd_stage1": [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, C.POINTER(_i32), _vp],
    "avsr_bn_partials_f64": [_vp, _i32, _i32, _vp, _vp],
    "avsr_bn_finalize_f64": [_vp, _i32, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "avsr_bn_bwd_finalize_f64": [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _vp],
    "avsr_bn_eval_affine": [_vp, _vp, _vp, _vp, _f32, _vp, _vp, _i32, _vp],
    "avsr_bn_finalize": [_vp, _i32, _i32, _i64, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "avsr_conv3d_supported": [C.POINTER(Conv3dDesc)],
    "avsr_conv3d_fwd": [C.POINTER(Conv3dDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i32), _vp],
    "avsr_conv3d_bwd_data": [C.POINTER(Conv3dDesc), _vp, _vp, _vp, _f32, _vp],
    "avsr_conv3d_bwd_weight": [C.POINTER(Conv3dDesc), _vp, _vp, _vp, _f32, _vp, _i64, _vp],
    "avsr_conv3d_bn_finalize": [_vp, _i32, _i32, _i64, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "avsr_logmel_supported": [_i32, _i32, _i32, _i32, _i32],
    "avsr_logmel_fwd": [C.POINTER(LogmelArgs), _vp],
    "avsr_spec_augment_supported": [_i32, _i32, _i32, _i32, _i32],
    "avsr_spec_augment": [C.POINTER(SpecAugmentArgs), _vp],
    "avsr_video_augment_supported": [_i32, _i32, _i32, _i32, _i32, _i32],
    "avsr_video_augment": [C.POINTER(VideoAugmentArgs), _vp],
    "avsr_ctc_loss": [C.POINTER(CtcArgs), _vp],
    "avsr_ctc_best_path": [_vp, _i64, _vp, _i32, _i32, _i32, _vp, _vp],
    "avsr_ctc_prefix_search_supported": [_i32, _i32, _i32],
    "avsr_ctc_prefix_search": [C.POINTER(CtcPrefixArgs), _vp],
    "avsr_ctc_prefix_lm_supported": [_i32, _i32, _i32, _i32, _i32, _i32, _i32],
    "avsr_ctc_prefix_search_lm": [C.POINTER(CtcPrefixArgs), C.POINTER(CtcPrefixLm), _vp],
    "avsr_ctc_prefix_ngram_supported": [_i32, _i32, _i32, _i32, _i32],
    "avsr_ctc_prefix_search_ngram": [C.POINTER(CtcPrefixArgs), C.POINTER(CtcPrefixNgram), _vp],
    "avsr_ctc_prefix_word_ngram_supported": [_i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32],
    "avsr_ctc_prefix_search_word_ngram": [C.POINTER(CtcPrefixArgs), C.POINTER(CtcPrefixWordNgram), _vp],
    "avsr_ctc_align_supported": [_i32, _i32],
    "avsr_ctc_align": [C.POINTER(CtcAlignArgs), _vp],
    "avsr_seq_logprob": [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _i64, _vp],
    "avsr_rescore_select": [_vp, _vp, _vp, _i32, _i32, _f32, _vp, _vp, _vp],
    "avsr_batchnorm_apply": [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp],
    "avsr_attn_rnn_bwd": [C.POINTER(AttnRnn), _vp],
    "avsr_beam_gather_tree": [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp],
    "avsr_beam_search_step": [_vp, _i32, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp],
    "avsr_beam_lm_supported": [C.POINTER(BeamLm)],
    "avsr_beam_lm_step": [C.POINTER(BeamLm), _vp, _vp, _i32, _i32, _vp],
    "avsr_beam_search_step_lm": [_vp, _i32, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp,
                                 _vp, _f32, _vp],
    "avsr_attn_rnn_fwd_lm": [C.POINTER(AttnRnn), C.POINTER(BeamLm), _i32, _i32, _vp],
    "avsr_beam_ngram_supported": [C.POINTER(BeamNgram)],
    "avsr_beam_ngram_step": [C.POINTER(BeamNgram), _vp, _vp, _i32, _i32, _vp],
    "avsr_attn_rnn_fwd_ngram": [C.POINTER(AttnRnn), C.POINTER(BeamNgram), C.POINTER(BeamCtc), _i32, _i32, _vp],
    "avsr_beam_word_ngram_supported": [C.POINTER(BeamWordNgram)],
    "avsr_beam_word_ngram_step": [C.POINTER(BeamWordNgram), _vp, _vp, _i32, _i32, _vp],
    "avsr_attn_rnn_fwd_word_ngram": [C.POINTER(AttnRnn), C.POINTER(BeamWordNgram), C.POINTER(BeamCtc), _i32, _i32, _vp],
    "avsr_beam_ctc_supported": [C.POINTER(BeamCtc)],
    "avsr_beam_ctc_begin": [C.POINTER(BeamCtc), _vp],
    "avsr_beam_ctc_step": [C.POINTER(BeamCtc), _vp, _vp, _vp, _i32, _vp],
    "avsr_beam_search_step_ctc": [_vp, _i32, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp,
                                  _vp, _f32, _vp, _f32, _vp, _vp],
    "avsr_attn_rnn_fwd_ctc": [C.POINTER(AttnRnn), C.POINTER(BeamLm), C.POINTER(BeamCtc), _i32, _i32, _vp],
    "avsr_attn_alpha_rows": [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp],
    "avsr_bahdanau_dkeys": [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp],
    "avsr_transpose": [C.POINTER(TransposeJob), _i32, _vp],
    "avsr_colsum": [C.POINTER(Mat), C.POINTER(Mat), _i32, _i32, _f32, _f32, _vp, _vp, _i64, _vp],
    "avsr_batchnorm_fwd": [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i64, _vp],
    "avsr_batchnorm_xhat": [_vp, _vp, _vp, _vp, _i32, _i32, _vp],
    "avsr_batchnorm_fwd_ex": [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _f32, _f32, _i32, _i32, _vp, _i64, _vp],
    "avsr_batchnorm_bwd": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _vp, _i64, _vp],
    "avsr_im2col": [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp],
    "avsr_col2im": [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _vp],
    "avsr_relu": [_vp, _vp, _i64, _vp],
    "avsr_relu_bwd": [_vp, _vp, _vp, _i64, _vp],
    "avsr_add": [_vp, _vp, _vp, _i64, _vp],
    "avsr_selu": [_vp, _vp, _i64, _vp],
    "avsr_selu_bwd": [_vp, _vp, _vp, _i64, _vp],
    "avsr_conv3x3_supported": [_i32, _i32, _i32, _i32],
    "avsr_conv3x3": [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _vp],
    "avsr_conv3x3_bwd_data_s2": [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _vp],
    "avsr_conv3x3_bwd_weight": [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _vp, _i64, _vp],
    "avsr_embed_labels": [_vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _vp],
    "avsr_embed_grad": [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _i64, _vp],
    "avsr_dropout_rows": [C.POINTER(Mat), C.POINTER(Mat), _i32, _i32, _vp, _i32, _f32, _i32, _i32, _i32, _vp],
    "avsr_seq_loss": [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _vp],
    "avsr_seq_loss_fun": [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _vp],
    "avsr_au_loss": [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _f32, _vp],
    "avsr_au_loss_dp": [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _f32, _vp, _vp],
    "avsr_normed_v": [_vp, _vp, _vp, _i32, _vp],
    "avsr_normed_v_bwd": [_vp, _vp, _vp, _vp, _vp, _i32, _vp],
    "avsr_reduce_scalar": [_vp, _i32, _vp, _i32, _i32, _f32, _vp],
    "avsr_l2_regularise": [C.POINTER(_i64), C.POINTER(_i64), _i32, _vp, _vp, _f32, _vp, _vp, _vp],
    "avsr_global_norm": [_vp, _i64, _f32, _vp, _vp, _vp],
    "avsr_adam_step": [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _f32, _i32, _f32, _f32, _vp],
    "avsr_batchnorm_sync_sum": [_vp, _i32, _i32, _vp, _vp, _i64, _vp],
    "avsr_batchnorm_sync_sqsum": [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _vp],
    "avsr_batchnorm_sync_apply": [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _f32, _i32, _vp],
    "avsr_batchnorm_sync_moments": [_vp, _i32, _i32, _vp, _vp, _i64, _vp],
    "avsr_dp_sync_unpack": [_vp, _vp, _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), _vp],
    "avsr_seq_loss_per_utterance": [_vp, _vp, _vp, _vp, _i32, _i32, _vp],
    "avsr_instnorm_fwd": [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _f32, _vp],
    "avsr_instnorm_bwd": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp],
    "avsr_optimiser_step": [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _f32, _i32, _i32, _f32, _f32, _i32, _f32, _vp],
    "avsr_highway_fwd": [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp],
    "avsr_highway_bwd": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp],
    "avsr_copy_words": [_vp, _vp, _i64, _vp],
    "avsr_zero_words": [_vp, _i64, _vp],
    "avsr_zero_multi": [C.POINTER(_vp), C.POINTER(_i64), _i32, _vp],
    "avsr_add_int": [_vp, _i32, _vp, _vp],
    "avsr_colsum_multi": [C.POINTER(ColsumJob), _i32, _vp, _i64, _vp],
    "avsr_slab_defer_begin": [], "avsr_slab_defer_end": [_vp],
    "avsr_adam_step_decay": [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _f32, _i32, _i32, _f32, _f32, _vp],
    "avsr_prof_begin": [_i32],
    "avsr_prof_end": [C.POINTER(_i32), C.POINTER(_f32), C.POINTER(C.c_double)],
}
# every symbol the library must export: the table above plus the nine whose return type load() sets on its own
EXPORTS = ["avsr_abi_version", "avsr_sizeof", "avsr_attn_rnn_fused_ws_floats", "avsr_conv3d_wgrad_scratch_floats", "avsr_ctc_ws_floats",
           "avsr_ctc_align_ws_bytes", "avsr_ctc_prefix_lm_ws_bytes", "avsr_spec_augment_ws_floats",
           "avsr_video_augment_ws_floats"] + list(_SIGS)

_lib = None


def lib_path():
    return _build.LIB


def load():
    """Load (building first if sources are newer and hipcc is available).  Raises if unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    # AVSR_LIB: load another build of the library (A/B timing of kernel variants: tools/build_variant.py); never set in product use
    path = os.environ.get("AVSR_LIB") or _build.LIB
    if path == _build.LIB and _build.needs_build():
        try:
            _build.build()
        except Exception as e:  # no hipcc on the box: fall through to a prebuilt .so if present
            if not os.path.exists(path):
                raise AvsrError("libavsr_hip.so is missing and could not be built: %s" % e)
    lib = C.CDLL(path)
    lib.avsr_abi_version.restype = C.c_int
    lib.avsr_sizeof.restype = C.c_int64
    lib.avsr_sizeof.argtypes = [C.c_char_p]
    for sym in EXPORTS:
        if not hasattr(lib, sym):
            raise AvsrError("libavsr_hip.so does not export %s" % sym)
    for name, at in _SIGS.items():
        fn = getattr(lib, name)
        fn.argtypes = at
        fn.restype = C.c_int
    lib.avsr_attn_rnn_fused_ws_floats.argtypes = [_i32, _i32, _i32]
    lib.avsr_attn_rnn_fused_ws_floats.restype = C.c_int64
    lib.avsr_conv3d_wgrad_scratch_floats.argtypes = [C.POINTER(Conv3dDesc)]
    lib.avsr_conv3d_wgrad_scratch_floats.restype = C.c_int64
    lib.avsr_ctc_ws_floats.argtypes = [_i32, _i32, _i32]
    lib.avsr_ctc_ws_floats.restype = C.c_int64
    lib.avsr_spec_augment_ws_floats.argtypes = [_i32, _i32, _i32]
    lib.avsr_spec_augment_ws_floats.restype = C.c_int64
    lib.avsr_video_augment_ws_floats.argtypes = [_i32, _i32, _i32, _i32, _i32]
    lib.avsr_video_augment_ws_floats.restype = C.c_int64
    lib.avsr_ctc_align_ws_bytes.argtypes = [_i32, _i32, _i32]
    lib.avsr_ctc_align_ws_bytes.restype = C.c_int64
    lib.avsr_ctc_prefix_lm_ws_bytes.argtypes = [_i32, _i32, _i32, _i32]
    lib.avsr_ctc_prefix_lm_ws_bytes.restype = C.c_int64
    for name, st in _STRUCTS.items():
        n = lib.avsr_sizeof(name.encode())
        if n != C.sizeof(st):
            raise AvsrError("ABI mismatch for %s: C %d vs ctypes %d" % (name, n, C.sizeof(st)))
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        raise AvsrError("%s failed with code %d" % (what, rc))


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream
