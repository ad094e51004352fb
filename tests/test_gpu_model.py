"""Model-level parity: full train step (fwd, BPTT, clip, Adam) and greedy decode through the C ABI vs the
CPU oracle.  "vs CPU restatement of TF-1.13.1 semantics; TF parity unpinned" (SURVEY.md 8c).

Tolerances: logits / loss / global norm 1e-4 absolute (north_star), gradients 2e-4 of the tensor's max
magnitude, greedy ids bit-exact."""
import dataclasses

import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = {
    "c1_audio_uni_luong": dict(architecture="unimodal", encoder_type="unidirectional", video_units=None, audio_units=(32,),
                               attention_type=(("scaled_luong",), ("scaled_luong",))),
    "audio_uni3_luong": dict(architecture="unimodal", encoder_type="unidirectional", video_units=None, audio_units=(32, 32, 32),
                             attention_type=(("luong",), ("luong",))),
    "c2_audio_bi_bahdanau": dict(architecture="unimodal", encoder_type="bidirectional", video_units=None, audio_units=(32, 32),
                                 attention_type=(("bahdanau",), ("bahdanau",))),
    "c3_video_bi_normed": dict(architecture="unimodal", encoder_type="bidirectional", video_units=(32, 32), audio_units=None,
                               attention_type=(("normed_bahdanau",), ("normed_bahdanau",)), regress_aus=True),
    "c4_bimodal_uni": dict(architecture="bimodal", encoder_type="unidirectional", video_units=(32,), audio_units=(32, 32),
                           attention_type=(("scaled_luong",), ("scaled_luong",)), regress_aus=True),
    "bimodal_bi_mixed": dict(architecture="bimodal", encoder_type="bidirectional", video_units=(16,), audio_units=(16, 16),
                             decoder_units=(32,), attention_type=(("normed_bahdanau",), ("bahdanau",))),
    "c5_av_align": dict(architecture="av_align", encoder_type="unidirectional", video_units=(32,), audio_units=(32, 32),
                        attention_type=(("scaled_luong",), ("scaled_luong",)), regress_aus=True),
    "av_align_1layer_bahdanau": dict(architecture="av_align", encoder_type="unidirectional", video_units=(32,), audio_units=(32,),
                                     attention_type=(("bahdanau",), ("luong",))),
    "gru_audio_uni": dict(architecture="unimodal", encoder_type="unidirectional", video_units=None, audio_units=(32, 32),
                          cell_type="gru", attention_type=(("scaled_luong",), ("scaled_luong",))),
    "gru_video_bi_bahdanau": dict(architecture="unimodal", encoder_type="bidirectional", video_units=(32, 32), audio_units=None,
                                  cell_type="gru", attention_type=(("bahdanau",), ("bahdanau",)), regress_aus=True),
    "gru_av_align": dict(architecture="av_align", encoder_type="unidirectional", video_units=(32,), audio_units=(32, 32),
                         cell_type="gru", attention_type=(("scaled_luong",), ("normed_bahdanau",))),
    # lip crops through video.resnet_cnn: [B, T, 36, 36, 3] frames, CNN BN in training mode, conv L2
    "c3_video_cnn_bi": dict(architecture="unimodal", encoder_type="bidirectional", video_units=(32, 32), audio_units=None,
                            attention_type=(("scaled_luong",), ("scaled_luong",)), regress_aus=True, video_processing="resnet_cnn",
                            cnn_filters=(8, 8, 16, 16), cnn_dense_units=16, video_feat=16),
    "c4_bimodal_cnn": dict(architecture="bimodal", encoder_type="unidirectional", video_units=(32,), audio_units=(32, 32),
                           attention_type=(("scaled_luong",), ("scaled_luong",)), regress_aus=True, video_processing="resnet_cnn",
                           cnn_filters=(8, 16, 32, 64), cnn_dense_units=16, video_feat=16),
    # input_dense_layers (encoder.py:148-171): SELU Dense stack between BN and the first RNN layer
    "bimodal_input_dense": dict(architecture="bimodal", encoder_type="unidirectional", video_units=(32,), audio_units=(32, 32),
                                attention_type=(("scaled_luong",), ("scaled_luong",)), regress_aus=True, input_dense_layers=(24, 16)),
    "av_align_1layer_dense": dict(architecture="av_align", encoder_type="unidirectional", video_units=(32,), audio_units=(32,),
                                  attention_type=(("bahdanau",), ("luong",)), input_dense_layers=(24,)),
    "video_cnn_dense_bi": dict(architecture="unimodal", encoder_type="bidirectional", video_units=(32, 32), audio_units=None,
                               attention_type=(("scaled_luong",), ("scaled_luong",)), video_processing="resnet_cnn",
                               cnn_filters=(8, 8, 16, 16), cnn_dense_units=16, video_feat=16, input_dense_layers=(24,)),
    "dense_no_bn": dict(architecture="unimodal", encoder_type="unidirectional", video_units=None, audio_units=(32, 32),
                        batch_normalisation=False, input_dense_layers=(16,)),
    # enable_attention=False (decoder_unimodal.py:320: plain decoder cell from the encoder's final state, no memory)
    "no_attention": dict(architecture="unimodal", encoder_type="unidirectional", video_units=None, audio_units=(32, 32),
                         enable_attention=False),
    "no_attention_gru_bi": dict(architecture="unimodal", encoder_type="bidirectional", video_units=None, audio_units=(32,),
                                cell_type="gru", enable_attention=False),
    # avsr.LM (lm.py:275-471): labels only -- embedding, decoder cell from the zero state, Dense(V), no warm-up
    "lm_lstm": dict(architecture="lm", video_units=None, audio_units=None, warmup_steps=0),
    "lm_gru": dict(architecture="lm", video_units=None, audio_units=None, cell_type="gru", warmup_steps=0),
    # the non-default per-step losses (seq2seq.py:147-163, avsr/devel.py): focal, multi-class, label smoothing
    "loss_focal": dict(architecture="unimodal", encoder_type="unidirectional", video_units=None, audio_units=(32,), loss_fun="focal_loss"),
    "loss_mc_bimodal": dict(architecture="bimodal", encoder_type="unidirectional", video_units=(32,), audio_units=(32,), loss_fun="mc_loss"),
    "label_smoothing": dict(architecture="unimodal", encoder_type="unidirectional", video_units=None, audio_units=(32,),
                            attention_type=(("bahdanau",), ("bahdanau",)), label_smoothing=0.1),
    # encoder_weight_sharing (cells.py:77): layers >= 2 reuse layer 1's variables; their gradients accumulate
    "weight_sharing_uni4": dict(architecture="unimodal", encoder_type="unidirectional", video_units=None, audio_units=(32, 32, 32, 32),
                                encoder_weight_sharing=True),
    "weight_sharing_uni_gru": dict(architecture="unimodal", encoder_type="unidirectional", video_units=(16, 16, 16), audio_units=None,
                                   decoder_units=(16,), cell_type="gru", encoder_weight_sharing=True,
                                   attention_type=(("bahdanau",), ("bahdanau",))),
    # ... and is silently ignored on bidirectional stacks (encoder.py:92-108 does not pass it): every layer owns its variables
    "weight_sharing_bi_gru_inert": dict(architecture="unimodal", encoder_type="bidirectional", video_units=(16, 16, 16), audio_units=None,
                                        cell_type="gru", encoder_weight_sharing=True, attention_type=(("bahdanau",), ("bahdanau",))),
    # multi-layer decoder cells (MultiRNNCell under the AttentionWrapper; decoder_unimodal.py:101-108, :151-157): layer 0 starts from
    # the encoder state, the layers above from zero; the TOP layer's output queries the attention
    "dec2_unimodal": dict(architecture="unimodal", encoder_type="unidirectional", video_units=None, audio_units=(32, 32),
                          decoder_units=(32, 32)),
    "dec3_bimodal_mixed": dict(architecture="bimodal", encoder_type="bidirectional", video_units=(16,), audio_units=(16, 16),
                               decoder_units=(32, 32, 32), attention_type=(("normed_bahdanau",), ("scaled_luong",))),
    "dec2_av_align": dict(architecture="av_align", encoder_type="unidirectional", video_units=(32,), audio_units=(32, 32),
                          decoder_units=(32, 32), attention_type=(("scaled_luong",), ("bahdanau",))),
    "dec2_lm": dict(architecture="lm", video_units=None, audio_units=None, decoder_units=(32, 32), warmup_steps=0),
    # ... with GRU cells (round 6): every layer runs its gate and candidate phases, the layer below reads both gradients of the one above
    "dec2_gru_unimodal": dict(architecture="unimodal", encoder_type="unidirectional", video_units=None, audio_units=(32, 32),
                              decoder_units=(32, 32), cell_type="gru"),
    "dec3_gru_av_align": dict(architecture="av_align", encoder_type="unidirectional", video_units=(32,), audio_units=(32, 32),
                              decoder_units=(32, 32, 32), cell_type="gru", attention_type=(("scaled_luong",), ("normed_bahdanau",))),
    "dec2_gru_lm": dict(architecture="lm", video_units=None, audio_units=None, decoder_units=(32, 32), cell_type="gru", warmup_steps=0),
    # residual_encoder (cells.py:91-92): ResidualWrapper on encoder layers > 0; those stacks run through the per-step launches
    "residual_uni3": dict(architecture="unimodal", encoder_type="unidirectional", video_units=None, audio_units=(32, 32, 32),
                          residual_encoder=True),
    "residual_bimodal_uni": dict(architecture="bimodal", encoder_type="unidirectional", video_units=(32, 32), audio_units=(32, 32, 32),
                                 decoder_units=(32,), residual_encoder=True),
    # ResidualWrapper around GRU cells (cells.py:89-92 wraps whatever _build_single_cell returned)
    "residual_gru_uni3": dict(architecture="unimodal", encoder_type="unidirectional", video_units=None, audio_units=(32, 32, 32),
                              cell_type="gru", residual_encoder=True),
    "residual_gru_av_align": dict(architecture="av_align", encoder_type="unidirectional", video_units=(32, 32, 32), audio_units=(32, 32),
                                  cell_type="gru", residual_encoder=True, attention_type=(("scaled_luong",), ("bahdanau",))),
    # inert on bidirectional stacks (encoder.py:92-108) -- unequal widths are therefore fine -- and on the AV-Align audio stack (:225-233)
    "residual_bimodal_bi_inert": dict(architecture="bimodal", encoder_type="bidirectional", video_units=(16, 16), audio_units=(16, 32, 16),
                                      decoder_units=(32,), residual_encoder=True),
    "residual_av_align_audio_inert": dict(architecture="av_align", encoder_type="unidirectional", video_units=(32, 32), audio_units=(16, 32, 32),
                                          residual_encoder=True, encoder_weight_sharing=True),
    # instance_normalisation (encoder.py:51-55): contrib.layers.instance_norm over the time axis, after the batch norm
    "instnorm_bimodal": dict(architecture="bimodal", encoder_type="unidirectional", video_units=(32,), audio_units=(32, 32),
                             instance_normalisation=True, regress_aus=True),
    "instnorm_only_bi": dict(architecture="unimodal", encoder_type="bidirectional", video_units=None, audio_units=(32,),
                             batch_normalisation=False, instance_normalisation=True, audio_feat=72),
    "instnorm_dense_av_align": dict(architecture="av_align", encoder_type="unidirectional", video_units=(32,), audio_units=(32,),
                                    instance_normalisation=True, input_dense_layers=(24,)),
    # the reference's other optimisers (seq2seq.py:195-218)
    "opt_nadam": dict(architecture="unimodal", encoder_type="unidirectional", video_units=None, audio_units=(32,), optimiser="Nadam"),
    "opt_adamw": dict(architecture="unimodal", encoder_type="unidirectional", video_units=None, audio_units=(32,), optimiser="AdamW",
                      weight_decay=0.01, recurrent_l2=None),
    "opt_momentum": dict(architecture="unimodal", encoder_type="unidirectional", video_units=None, audio_units=(32,), optimiser="Momentum",
                         warmup_steps=0),
    # highway_encoder (cells.py:89-90): HighwayWrapper on encoder layers > 0; those encoders run layer by layer with hoisted inputs
    "highway_uni3": dict(architecture="unimodal", encoder_type="unidirectional", video_units=None, audio_units=(32, 32, 32),
                         highway_encoder=True),
    "highway_bimodal_uni": dict(architecture="bimodal", encoder_type="unidirectional", video_units=(32, 32), audio_units=(32, 32, 32),
                                decoder_units=(32,), highway_encoder=True, regress_aus=True),
    "highway_bimodal_bi_inert": dict(architecture="bimodal", encoder_type="bidirectional", video_units=(16, 16), audio_units=(16, 16, 16),
                                     decoder_units=(32,), highway_encoder=True, regress_aus=True),
    "highway_av_align": dict(architecture="av_align", encoder_type="unidirectional", video_units=(32, 32), audio_units=(32,),
                             highway_encoder=True, residual_encoder=True),
    "highway_av_align_audio3": dict(architecture="av_align", encoder_type="unidirectional", video_units=(32, 32), audio_units=(16, 32, 32),
                                    highway_encoder=True),       # video stack highway, the 3-layer audio stack plain
    # HighwayWrapper around GRU cells (layer by layer, both input projections of every layer hoisted)
    "highway_gru_uni3": dict(architecture="unimodal", encoder_type="unidirectional", video_units=None, audio_units=(32, 32, 32),
                             cell_type="gru", highway_encoder=True),
    "highway_gru_av_align": dict(architecture="av_align", encoder_type="unidirectional", video_units=(32, 32), audio_units=(32, 32),
                                 cell_type="gru", highway_encoder=True, regress_aus=True),
    "no_bn_no_clip": dict(architecture="unimodal", encoder_type="unidirectional", video_units=None, audio_units=(32,),
                          batch_normalisation=False, clip_gradients=False, recurrent_l2=None, warmup_steps=0),
}


def make(case, B=5, Ta=21, Tv=9, L=7, ragged=True, seed=2001, batch_seed=1000, **over):
    from avsr_tf1_amd.config import ModelConfig
    from oracle import avsr_oracle as O
    kw = dict(decoder_units=(32,), embedding_size=16, video_feat=12, audio_feat=20)
    kw.update(CASES[case])
    kw.update(over)
    ocfg = O.OracleConfig(**kw)
    mcfg = ModelConfig(**{f.name: getattr(ocfg, f.name) for f in dataclasses.fields(ModelConfig) if hasattr(ocfg, f.name)})
    W = O.init_params(ocfg, seed=seed)
    # non-trivial biases / BN parameters so that every term is exercised
    rng = np.random.default_rng(7)
    for k in W:
        if k.endswith(("bias", "/b", "beta")):
            W[k] = (rng.standard_normal(W[k].shape) * 0.1).astype(np.float32)
        if k.endswith("gamma"):
            W[k] = (1.0 + rng.standard_normal(W[k].shape) * 0.1).astype(np.float32)
        if k.endswith("/g"):
            W[k] = (W[k] * 1.3).astype(np.float32)
    batch = O.synthetic_batch(ocfg, B=B, T_a=Ta, T_v=Tv, L=L, ragged=ragged, seed=batch_seed)
    return O, ocfg, mcfg, W, batch


@pytest.mark.parametrize("case", list(CASES))
def test_train_step_parity(case):
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    O, ocfg, mcfg, W, batch = make(case)
    ref = O.train_step(W, None, ocfg, batch)
    model = Seq2SeqModel(mcfg, weights=W)
    dbatch = Batch.from_numpy(batch)
    logits = model.forward_train(dbatch)
    torch.cuda.synchronize()
    lg = logits.cpu().numpy()
    assert np.isfinite(lg).all()
    assert np.abs(lg - ref["logits"]).max() < 1e-4, np.abs(lg - ref["logits"]).max()
    model.backward()
    model.apply_update()
    torch.cuda.synchronize()
    assert abs(float(model.loss.item()) - ref["loss"]) < 1e-4, (float(model.loss.item()), ref["loss"])
    assert abs(float(model.gnorm.item()) - ref["global_norm"]) < 1e-4 * max(1.0, ref["global_norm"])
    grads = model.export_tf_weights("grads")
    for k, g in ref["grads"].items():
        scale = max(1e-3, np.abs(g).max())
        err = np.abs(grads[k] - g).max()
        assert err < 2e-4 * scale + 1e-6, (k, err, scale)
    newp = model.export_tf_weights("params")
    for k, v in ref["params"].items():
        err = np.abs(newp[k] - v).max()
        assert err < 2e-5, (k, err)     # one Adam step moves each weight by <= lr_t ~ 4e-5 at step 1 of warm-up


@pytest.mark.parametrize("case", [c for c in CASES if not c.startswith("lm_") and c not in ("dec2_lm", "dec2_gru_lm")])
def test_greedy_decode_parity(case):
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    O, ocfg, mcfg, W, batch = make(case)
    # a few training steps of the oracle make EOS reachable for some utterances; decode must agree exactly
    ids_ref, lg_ref = O.greedy_decode(W, ocfg, batch, max_steps=12, return_logits=True)
    model = Seq2SeqModel(mcfg, weights=W)
    ids = model.greedy_decode(Batch.from_numpy(batch), max_steps=12).cpu().numpy()
    assert ids.shape == ids_ref.shape, (ids.shape, ids_ref.shape)
    assert (ids == ids_ref).all()
    ws, t_out = model._last_greedy
    lg = ws["dec"]["logits"][:, :t_out].cpu().numpy()
    assert np.abs(lg - lg_ref).max() < 1e-4


def test_second_step_and_eos_path():
    """Two consecutive train steps (Adam state, BN moving averages) and a decode where EOS fires early."""
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    O, ocfg, mcfg, W, batch = make("c4_bimodal_uni")
    r1 = O.train_step(W, None, ocfg, batch)
    r2 = O.train_step(r1["params"], r1["opt"], ocfg, batch)
    model = Seq2SeqModel(mcfg, weights=W)
    db = Batch.from_numpy(batch)
    model.train_step(db)
    loss2, gn2 = model.train_step(db)
    torch.cuda.synchronize()
    assert abs(float(loss2.item()) - r2["loss"]) < 1e-4
    newp = model.export_tf_weights("params")
    for k, v in r2["params"].items():
        assert np.abs(newp[k] - v).max() < 5e-5, k
    # force EOS: bias the output layer towards EOS so every utterance finishes at step 0 or 1
    W2 = {k: v.copy() for k, v in r2["params"].items()}
    W2["dec/out/bias"][ocfg.eos_id] += 3.0
    ids_ref = O.greedy_decode(W2, ocfg, batch, max_steps=10)
    m2 = Seq2SeqModel(mcfg, weights=W2)
    ids = m2.greedy_decode(db, max_steps=10).cpu().numpy()
    assert ids.shape == ids_ref.shape and (ids == ids_ref).all()


# ------------------------------------------------------------------------------------------------
# train-time stochastic wrappers: DropoutWrapper (cells.py:46-54) and scheduled sampling (decoder_*.py).  The masks and
# draws come from the stateless hash RNG shared bit-for-bit by the oracle and the kernels, so parity stays exact.
STOCH = [
    ("c1_audio_uni_luong", dict(use_dropout=True)),
    ("audio_uni3_luong", dict(use_dropout=True, sampling_probability=0.3)),
    ("c2_audio_bi_bahdanau", dict(use_dropout=True, sampling_probability=0.3)),
    ("c4_bimodal_uni", dict(use_dropout=True, sampling_probability=0.25)),
    ("bimodal_bi_mixed", dict(use_dropout=True, audio_dropout=(0.8, 0.9, 0.7), video_dropout=(1.0, 0.9, 0.9), decoder_dropout=(0.9, 0.8, 1.0))),
    ("c5_av_align", dict(use_dropout=True, sampling_probability=0.3)),
    ("av_align_1layer_bahdanau", dict(use_dropout=True)),
    ("c4_bimodal_uni", dict(sampling_probability=0.5)),
    ("gru_audio_uni", dict(use_dropout=True, sampling_probability=0.3)),
    ("gru_video_bi_bahdanau", dict(use_dropout=True)),
    ("gru_av_align", dict(use_dropout=True, sampling_probability=0.3)),
    ("bimodal_input_dense", dict(use_dropout=True, sampling_probability=0.2)),
    ("av_align_1layer_dense", dict(use_dropout=True)),
    ("video_cnn_dense_bi", dict(use_dropout=True)),
    ("no_attention", dict(use_dropout=True, sampling_probability=0.3)),
    ("lm_lstm", dict(use_dropout=True, sampling_probability=0.1)),
    ("label_smoothing", dict(use_dropout=True, sampling_probability=0.3)),
    ("loss_focal", dict(sampling_probability=0.3)),
    ("weight_sharing_uni4", dict(use_dropout=True)),
    ("dec2_unimodal", dict(use_dropout=True, sampling_probability=0.3)),
    ("dec3_bimodal_mixed", dict(use_dropout=True, decoder_dropout=(0.8, 0.9, 0.7))),
    ("dec2_av_align", dict(use_dropout=True, sampling_probability=0.2)),
    ("dec2_lm", dict(use_dropout=True, sampling_probability=0.1)),
    ("dec2_gru_unimodal", dict(use_dropout=True, sampling_probability=0.3)),
    ("dec3_gru_av_align", dict(use_dropout=True, decoder_dropout=(0.8, 0.9, 0.7))),
    ("dec2_gru_lm", dict(use_dropout=True, sampling_probability=0.1)),
    ("residual_uni3", dict(use_dropout=True)),
    ("highway_uni3", dict(use_dropout=True, sampling_probability=0.2)),
    ("highway_bimodal_uni", dict(use_dropout=True, video_dropout=(0.8, 0.9, 0.7))),
    ("opt_nadam", dict(use_dropout=True)),
    ("opt_adamw", dict(use_dropout=True)),
    ("opt_momentum", dict(use_dropout=True)),
    ("instnorm_bimodal", dict(use_dropout=True, sampling_probability=0.2)),
    ("residual_bimodal_uni", dict(use_dropout=True, audio_dropout=(0.8, 0.9, 0.7))),
    ("residual_gru_uni3", dict(use_dropout=True, sampling_probability=0.2)),
    ("highway_gru_uni3", dict(use_dropout=True, sampling_probability=0.2)),
    ("highway_gru_av_align", dict(use_dropout=True, video_dropout=(0.8, 0.9, 0.7))),
    ("residual_gru_av_align", dict(use_dropout=True, video_dropout=(0.8, 0.9, 0.7))),
]


@pytest.mark.parametrize("case,over", STOCH)
def test_train_step_parity_with_dropout_and_sampling(case, over):
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    O, ocfg, mcfg, W, batch = make(case, **over)
    r1 = O.train_step(W, None, ocfg, batch)
    r2 = O.train_step(r1["params"], r1["opt"], ocfg, batch)          # second step: new seed -> new masks
    model = Seq2SeqModel(mcfg, weights=W)
    db = Batch.from_numpy(batch)
    logits = model.forward_train(db)
    torch.cuda.synchronize()
    ws = model._cur[0]
    # tokens fed to VALID steps must agree exactly (draws for already-finished rows feed frozen steps: don't-care)
    consumed = np.arange(batch.labels.shape[1])[None, :] < batch.labels_len[:, None]
    assert (ws["dec"]["fed"].cpu().numpy()[consumed] == r1["fed_tokens"][consumed]).all()
    assert np.abs(logits.cpu().numpy() - r1["logits"]).max() < 1e-4
    model.backward()
    model.apply_update()
    torch.cuda.synchronize()
    assert abs(float(model.loss.item()) - r1["loss"]) < 1e-4
    assert abs(float(model.gnorm.item()) - r1["global_norm"]) < 1e-4 * max(1.0, r1["global_norm"])
    grads = model.export_tf_weights("grads")
    for k, g in r1["grads"].items():
        scale = max(1e-3, np.abs(g).max())
        assert np.abs(grads[k] - g).max() < 2e-4 * scale + 1e-6, k
    loss2, _ = model.train_step(db)
    torch.cuda.synchronize()
    assert abs(float(loss2.item()) - r2["loss"]) < 2e-4
    # eval graph: no dropout
    ids_ref = O.greedy_decode(r2["params"], ocfg, batch, max_steps=8)
    assert (model.greedy_decode(db, max_steps=8).cpu().numpy() == ids_ref).all()


# ------------------------------------------------------------------------------------------------
# full-width encoders (BASELINE configs[3] widths, short sequences): at 256 units and 64 utterances the persistent
# kernels run with all four 16-row groups, both XCDs of every pair and a crossing layer edge; the same case through
# the per-step launches (mode 0) keeps that path covered at width.  Both are checked against the oracle.
FULL_WIDTH = [
    ("c4_bimodal_uni", dict(video_units=(256,), audio_units=(256, 256, 256), decoder_units=(256,), embedding_size=128,
                            video_feat=128, audio_feat=80, use_dropout=True, sampling_probability=0.1)),
    ("c2_audio_bi_bahdanau", dict(audio_units=(256, 256, 256), decoder_units=(256,), embedding_size=128, audio_feat=80)),
    ("c5_av_align", dict(video_units=(256,), audio_units=(256, 256), decoder_units=(256,), embedding_size=128,
                         video_feat=128, audio_feat=80, use_dropout=True)),
]


# BASELINE configs[2] (visual-only, lip-CNN (8,16,32,64) -> 128 -> 2 x bi-LSTM-256) and configs[4] (AV-Align at B = 128: two 64-row
# slices of the persistent kernels), short sequences so that the fp64 oracle finishes in seconds
WIDE_EXTRA = [
    ("c3_video_cnn_bi", dict(video_units=(256, 256), decoder_units=(256,), embedding_size=128, cnn_filters=(8, 16, 32, 64),
                             cnn_dense_units=128, video_feat=128), dict(B=3, Ta=4, Tv=7, L=5)),
    ("c5_av_align", dict(video_units=(256,), audio_units=(256, 256, 256), decoder_units=(256,), embedding_size=128,
                         video_feat=128, audio_feat=80, use_dropout=True, sampling_probability=0.1), dict(B=128, Ta=14, Tv=6, L=4)),
]


@pytest.mark.parametrize("case,over,shape", WIDE_EXTRA)
def test_baseline_widths_c3_cnn_and_c5_b128(case, over, shape):
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    O, ocfg, mcfg, W, batch = make(case, **shape, **over)
    ref = O.train_step(W, None, ocfg, batch)
    model = Seq2SeqModel(mcfg, weights=W)
    db = Batch.from_numpy(batch)
    logits = model.forward_train(db)
    model.backward()
    model.apply_update()
    torch.cuda.synchronize()
    assert not model.check_persistent()
    assert np.abs(logits.cpu().numpy() - ref["logits"]).max() < 1e-4
    assert abs(float(model.loss.item()) - ref["loss"]) < 1e-4
    assert abs(float(model.gnorm.item()) - ref["global_norm"]) < 1e-4 * max(1.0, ref["global_norm"])
    grads = model.export_tf_weights("grads")
    for k, g in ref["grads"].items():
        scale = max(1e-3, np.abs(g).max())
        assert np.abs(grads[k] - g).max() < 2e-4 * scale + 1e-6, k
    ids_ref = O.greedy_decode(ref["params"], ocfg, batch, max_steps=6)
    assert (model.greedy_decode(db, max_steps=6).cpu().numpy() == ids_ref).all()


@pytest.mark.parametrize("mode", ["0", "3"])         # per-step launches / the persistent kernels
@pytest.mark.parametrize("case,over", FULL_WIDTH)
def test_full_width_train_step(case, over, mode, monkeypatch):
    from avsr_tf1_amd import ops
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    monkeypatch.setenv("AVSR_PERSISTENT_RNN", mode)
    O, ocfg, mcfg, W, batch = make(case, B=64, Ta=26, Tv=9, L=5, **over)
    ref = O.train_step(W, None, ocfg, batch)
    try:
        model = Seq2SeqModel(mcfg, weights=W)
        db = Batch.from_numpy(batch)
        logits = model.forward_train(db)
        model.backward()
        model.apply_update()
        torch.cuda.synchronize()
        assert not ops.rnn_persistent_error()
    finally:
        ops.rnn_set_persistent(False)
    assert np.abs(logits.cpu().numpy() - ref["logits"]).max() < 1e-4
    assert abs(float(model.loss.item()) - ref["loss"]) < 1e-4
    assert abs(float(model.gnorm.item()) - ref["global_norm"]) < 1e-4 * max(1.0, ref["global_norm"])
    grads = model.export_tf_weights("grads")
    for k, g in ref["grads"].items():
        scale = max(1e-3, np.abs(g).max())
        assert np.abs(grads[k] - g).max() < 2e-4 * scale + 1e-6, k


# ------------------------------------------------------------------------------------------------
# beam search (the reference's default decoding_algorithm, avsr.py:58): engine vs the oracle restatement
@pytest.mark.parametrize("case", ["c1_audio_uni_luong", "c2_audio_bi_bahdanau", "c4_bimodal_uni", "c5_av_align", "gru_audio_uni", "dec2_unimodal",
                                  "dec3_bimodal_mixed", "dec2_gru_unimodal", "dec3_gru_av_align"])
@pytest.mark.parametrize("K", [1, 4])
def test_beam_search_parity(case, K):
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    O, ocfg, mcfg, W, batch = make(case)
    r = O.train_step(W, None, ocfg, batch)                     # move off the all-uniform initial distribution
    W2 = {k: v.copy() for k, v in r["params"].items()}
    W2["dec/out/bias"][ocfg.eos_id] += 1.2                     # EOS reachable within a few steps, not immediately
    ref = O.beam_search_decode(W2, ocfg, batch, beam_width=K, max_steps=14, return_all=True)[0]
    model = Seq2SeqModel(mcfg, weights=W2)
    out = model.beam_search_decode(Batch.from_numpy(batch), beam_width=K, max_steps=14, check_every=3, return_all=True).cpu().numpy()
    assert out.shape == ref.shape, (out.shape, ref.shape)
    assert (out == ref).all()
    if K == 1:                                                  # width-1 beam search == greedy up to the EOS padding convention
        g = O.greedy_decode(W2, ocfg, batch, max_steps=14)
        T = min(g.shape[1], ref.shape[1])
        gg = np.where(np.cumsum(g[:, :T] == ocfg.eos_id, axis=1) - (g[:, :T] == ocfg.eos_id) > 0, ocfg.eos_id, g[:, :T])
        assert (gg == ref[:, :T, 0]).all()


# ------------------------------------------------------------------------------------------------
# data-parallel algebra on ONE GPU: two engine instances hold the two halves of a batch, the test plays RCCL (sums the
# buffers the trainer would all-reduce).  With sync batch-norm the summed gradients, loss and moving statistics must be
# those of ONE engine on the whole batch; the real 2-process collective logic is tests/test_dp_gloo.py.
@pytest.mark.parametrize("case", ["c4_bimodal_uni", "c2_audio_bi_bahdanau", "c5_av_align"])
def test_two_shards_with_sync_bn_equal_whole_batch(case):
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    O, ocfg, mcfg, W, batch = make(case, B=6, ragged=True, regress_aus=False)
    whole = Seq2SeqModel(mcfg, weights=W)
    whole.forward_train(Batch.from_numpy(batch))
    whole.backward()
    torch.cuda.synchronize()

    def shard(lo, hi):
        return O.Batch(**{k: (None if getattr(batch, k) is None else np.ascontiguousarray(getattr(batch, k)[lo:hi]))
                          for k in ("audio", "audio_len", "video", "video_len", "aus", "labels", "labels_len")})
    models = [Seq2SeqModel(mcfg, weights=W) for _ in range(2)]
    shards = [Batch.from_numpy(shard(0, 2)), Batch.from_numpy(shard(2, 6))]          # unequal shards on purpose
    for m in models:
        assert m.bn_sync_enable() is not None
    L = batch.labels.shape[1]
    denom = float(np.minimum(batch.labels_len, L).sum())
    tot = sum(m.bn_sync_sums(b).clone() for m, b in zip(models, shards))
    for m in models:
        m.bn_sync["sum"].copy_(tot)
    tot = sum(m.bn_sync_squares(b).clone() for m, b in zip(models, shards))
    for m, b in zip(models, shards):
        m.bn_sync["sq"].copy_(tot)
        m.denom.fill_(denom)
        m.forward_train(b, compute_denom=False)
        m.backward()
    torch.cuda.synchronize()
    g = models[0].grads + models[1].grads
    gw = whole.grads
    assert float((g - gw).abs().max()) < 2e-5 * max(1.0, float(gw.abs().max())), float((g - gw).abs().max())
    assert abs(float(models[0].loss.item() + models[1].loss.item()) - float(whole.loss.item())) < 1e-4
    for s in mcfg.streams():
        for k in ("moving_mean", "moving_variance"):
            a, b_ = whole.export_tf_weights("params")[f"{s}/bn/{k}"], models[1].export_tf_weights("params")[f"{s}/bn/{k}"]
            assert np.abs(a - b_).max() < 1e-6, (s, k)


# ------------------------------------------------------------------------------------------------
# edge shapes: a single utterance, one-frame / one-token sequences, utterances at the minimum length next to full ones,
# zero-length memories (an all-padding row), and a batch wider than one 64-row slice of the persistent kernels
def _edge_batch(O, ocfg, B, Ta, Tv, L, alen, vlen, llen):
    b = O.synthetic_batch(ocfg, B=B, T_a=Ta, T_v=Tv, L=L, ragged=False)
    if b.audio is not None:
        b.audio_len = np.asarray(alen, np.int32)
        b.audio *= (np.arange(Ta)[None, :, None] < b.audio_len[:, None, None])
    if b.video is not None:
        b.video_len = np.asarray(vlen, np.int32)
        b.video *= (np.arange(Tv)[None, :, None] < b.video_len[:, None, None])
    b.labels_len = np.asarray(llen, np.int32)
    for i in range(B):
        b.labels[i, b.labels_len[i] - 1] = ocfg.eos_id
        b.labels[i, b.labels_len[i]:] = 0
    return b


EDGE = [
    ("c1_audio_uni_luong", dict(B=1, Ta=1, Tv=1, L=1, alen=[1], vlen=[1], llen=[1])),
    ("c4_bimodal_uni", dict(B=1, Ta=9, Tv=3, L=4, alen=[9], vlen=[3], llen=[4])),
    ("c4_bimodal_uni", dict(B=3, Ta=12, Tv=5, L=6, alen=[1, 12, 7], vlen=[5, 1, 2], llen=[6, 1, 2])),
    ("c2_audio_bi_bahdanau", dict(B=3, Ta=10, Tv=4, L=5, alen=[1, 10, 2], vlen=[1, 1, 1], llen=[1, 5, 3])),
    ("c5_av_align", dict(B=2, Ta=8, Tv=4, L=3, alen=[8, 1], vlen=[1, 4], llen=[3, 1])),
    ("gru_av_align", dict(B=2, Ta=6, Tv=3, L=3, alen=[1, 6], vlen=[3, 1], llen=[1, 3])),
    ("c3_video_bi_normed", dict(B=2, Ta=4, Tv=7, L=4, alen=[4, 4], vlen=[1, 7], llen=[4, 2])),
    ("c4_bimodal_uni", dict(B=67, Ta=6, Tv=3, L=3, alen=[6] * 30 + [1] * 7 + [3] * 30, vlen=[3] * 40 + [1] * 27, llen=[3] * 50 + [1] * 17)),
]


@pytest.mark.parametrize("case,shape", EDGE)
def test_edge_shapes_train_and_greedy(case, shape):
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    O, ocfg, mcfg, W, _ = make(case, B=2)
    batch = _edge_batch(O, ocfg, **shape)
    ref = O.train_step(W, None, ocfg, batch)
    model = Seq2SeqModel(mcfg, weights=W)
    db = Batch.from_numpy(batch)
    logits = model.forward_train(db)
    model.backward()
    model.apply_update()
    torch.cuda.synchronize()
    assert np.abs(logits.cpu().numpy() - ref["logits"]).max() < 1e-4
    assert abs(float(model.loss.item()) - ref["loss"]) < 1e-4
    assert abs(float(model.gnorm.item()) - ref["global_norm"]) < 1e-4 * max(1.0, ref["global_norm"])
    grads = model.export_tf_weights("grads")
    for k, g in ref["grads"].items():
        scale = max(1e-3, np.abs(g).max())
        assert np.abs(grads[k] - g).max() < 2e-4 * scale + 1e-6, k
    ids_ref = O.greedy_decode(ref["params"], ocfg, batch, max_steps=6)
    ids = model.greedy_decode(db, max_steps=6).cpu().numpy()
    assert ids.shape == ids_ref.shape and (ids == ids_ref).all()


# ------------------------------------------------------------------------------------------------
# alignment_history of the greedy decode (write_attention_alignment=True): decoder mechanisms + the AV-Align layer
@pytest.mark.parametrize("case", ["c1_audio_uni_luong", "c2_audio_bi_bahdanau", "c3_video_bi_normed", "c4_bimodal_uni", "bimodal_bi_mixed",
                                  "c5_av_align", "av_align_1layer_bahdanau", "gru_av_align"])
def test_greedy_attention_alignments(case):
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    O, ocfg, mcfg, W, batch = make(case)
    r1 = O.train_step(W, None, ocfg, batch)
    W2 = {k: v.copy() for k, v in r1["params"].items()}
    W2["dec/out/bias"][ocfg.eos_id] += 1.5                       # some utterances finish early -> zero rows after EOS
    ids_ref, al_ref = O.greedy_decode(W2, ocfg, batch, max_steps=9, return_alignments=True)
    model = Seq2SeqModel(mcfg, weights=W2)
    ids = model.greedy_decode(Batch.from_numpy(batch), max_steps=9).cpu().numpy()
    assert (ids == ids_ref).all()
    al = model.attention_alignments()
    assert al is model.attention_alignments()                    # idempotent (scores are normalised in place once)
    assert len(al["decoder"]) == len(al_ref["decoder"])
    for a, r in zip(al["decoder"], al_ref["decoder"]):
        a = a.cpu().numpy()
        assert a.shape == r.shape and np.abs(a - r).max() < 1e-5
        live = r.sum(-1) > 0
        assert np.abs(a.sum(-1)[live] - 1.0).max() < 1e-5        # rows of a live step sum to one over the valid frames
    if ocfg.architecture == "av_align":
        a = al["encoder"].cpu().numpy()
        assert a.shape == al_ref["encoder"].shape and np.abs(a - al_ref["encoder"]).max() < 1e-5
    else:
        assert al["encoder"] is None


@pytest.mark.parametrize("case", ["lm_lstm", "lm_gru", "dec2_lm", "dec2_gru_lm"])
def test_lm_sequence_likelihoods(case):
    """The language model's evaluate graph: per-utterance average step loss of a teacher-forced pass (lm.py:390-401)."""
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    O, ocfg, mcfg, W, batch = make(case, B=7, L=9)
    ref = O.lm_likelihoods(W, ocfg, batch)
    got = Seq2SeqModel(mcfg, weights=W).sequence_likelihoods(Batch.from_numpy(batch)).cpu().numpy()
    assert got.shape == ref.shape and np.abs(got - ref).max() < 1e-5


# ------------------------------------------------------------------------------------------------
# BASELINE configs at their FULL sequence lengths and widths (T_a = 500 x 80, T_v = 75 x 128, T_dec = 40, 256 units), 8 ragged
# utterances so that the fp64 oracle finishes in seconds: the 500-step recurrences, the persistent kernels' full time loops and
# the 40-step decoder are compared directly (no size-independent proxy needed).
FULL_LENGTH = [
    ("c4_bimodal_uni", dict(video_units=(256,), audio_units=(256, 256, 256), decoder_units=(256,), embedding_size=128,
                            video_feat=128, audio_feat=80, regress_aus=True)),
    ("c5_av_align", dict(video_units=(256,), audio_units=(256, 256), decoder_units=(256,), embedding_size=128,
                         video_feat=128, audio_feat=80, regress_aus=True)),
    ("c2_audio_bi_bahdanau", dict(audio_units=(256, 256, 256), decoder_units=(256,), embedding_size=128, audio_feat=80)),
]


# 8 ragged utterances = one whole 8-row group of the persistent kernels (about a second of oracle time per case with the capped pool;
# the whole batch at these lengths: FULL_SIZE below)
@pytest.mark.parametrize("case,over", FULL_LENGTH)
def test_full_length_train_step_and_greedy(case, over):
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    nb = 8
    O, ocfg, mcfg, W, batch = make(case, B=nb, Ta=500, Tv=75, L=40, ragged=True, **over)
    ref = O.train_step(W, None, ocfg, batch)
    model = Seq2SeqModel(mcfg, weights=W)
    db = Batch.from_numpy(batch)
    logits = model.forward_train(db)
    model.backward()
    model.apply_update()
    torch.cuda.synchronize()
    assert not model.check_persistent()
    assert np.abs(logits.cpu().numpy() - ref["logits"]).max() < 1e-4
    assert abs(float(model.loss.item()) - ref["loss"]) < 1e-4
    assert abs(float(model.gnorm.item()) - ref["global_norm"]) < 1e-4 * max(1.0, ref["global_norm"])
    grads = model.export_tf_weights("grads")
    for k, g in ref["grads"].items():
        scale = max(1e-3, np.abs(g).max())
        assert np.abs(grads[k] - g).max() < 5e-4 * scale + 1e-6, (k, np.abs(grads[k] - g).max(), scale)
    ids_ref = O.greedy_decode(ref["params"], ocfg, batch, max_steps=40)
    ids = model.greedy_decode(db, max_steps=40).cpu().numpy()
    assert ids.shape == ids_ref.shape and (ids == ids_ref).all()


# ------------------------------------------------------------------------------------------------
# Every BASELINE config at its FULL size -- whole batch, full lengths, full widths, lip crops through the CNN front-end where the config
# has a video stream, DropoutWrapper + scheduled sampling ON as in the reference's defaults (avsr/avsr.py:51-56) and in bench.py -- one
# train step and the greedy decode against the fp64 oracle.  (Round 6: affordable in the default suite once the oracle's thread pool is
# capped at the container's CPU budget, tests/conftest.py: 3-10 s of oracle time per case on the GPU box.)  c4 is bench.py's headline
# workload to the letter; c5 runs B = 128 (two 64-row slices of the persistent kernels, 128 rows of the attentive layer's launch).
_W256 = dict(decoder_units=(256,), embedding_size=128, audio_feat=80, video_feat=128, use_dropout=True, sampling_probability=0.1)
_CNN = dict(video_processing="resnet_cnn", cnn_filters=(8, 16, 32, 64), cnn_dense_units=128)
FULL_SIZE = [
    ("c2_audio_bi_bahdanau", dict(audio_units=(256, 256, 256), **_W256), 64),
    ("c3_video_cnn_bi", dict(video_units=(256, 256), **_W256, **_CNN), 64),
    ("c4_bimodal_cnn", dict(video_units=(256,), audio_units=(256, 256, 256), **_W256, **_CNN), 64),
    ("c5_av_align", dict(video_units=(256,), audio_units=(256, 256, 256), regress_aus=True, **_W256, **_CNN), 128),
]


@pytest.mark.parametrize("case,over,nb", FULL_SIZE, ids=[c[0] + "_B%d" % c[2] for c in FULL_SIZE])
def test_full_size_train_step_and_greedy(case, over, nb):
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    O, ocfg, mcfg, W, batch = make(case, B=nb, Ta=500, Tv=75, L=40, ragged=True, **over)
    ref = O.train_step(W, None, ocfg, batch)
    model = Seq2SeqModel(mcfg, weights=W)
    db = Batch.from_numpy(batch)
    logits = model.forward_train(db)
    torch.cuda.synchronize()
    consumed = np.arange(batch.labels.shape[1])[None, :] < batch.labels_len[:, None]
    assert (model._cur[0]["dec"]["fed"].cpu().numpy()[consumed] == ref["fed_tokens"][consumed]).all()
    model.backward()
    model.apply_update()
    torch.cuda.synchronize()
    assert not model.check_persistent()
    lg = logits.cpu().numpy()
    assert np.isfinite(lg).all()
    assert np.abs(lg - ref["logits"]).max() < 1e-4, np.abs(lg - ref["logits"]).max()
    assert abs(float(model.loss.item()) - ref["loss"]) < 1e-4, (float(model.loss.item()), ref["loss"])
    assert abs(float(model.gnorm.item()) - ref["global_norm"]) < 1e-4 * max(1.0, ref["global_norm"])
    grads = model.export_tf_weights("grads")
    for k, g in ref["grads"].items():
        scale = max(1e-3, np.abs(g).max())
        # a convolution kernel's gradient is an fp32 sum over every position of every frame (B = 128: 9600 frames, 3.1 M terms on the
        # 18x18 maps) of products that largely cancel (|sum| ~ 2e-3): 2e-3 of the tensor's largest entry there, 5e-4 everywhere else
        rel = 2e-3 if "/cnn/" in k else 5e-4
        assert np.abs(grads[k] - g).max() < rel * scale + 1e-6, (k, np.abs(grads[k] - g).max(), scale)
    ids_ref = O.greedy_decode(ref["params"], ocfg, batch, max_steps=40)
    ids = model.greedy_decode(db, max_steps=40).cpu().numpy()
    assert ids.shape == ids_ref.shape and (ids == ids_ref).all()


def test_rank_seed_offset_decorrelates_dropout_masks():
    """Data-parallel ranks key the stateless RNG with step + (rank << 24): same weights and batch, different masks; offset 0 is the oracle's stream."""
    from avsr_tf1_amd.model import Batch, Seq2SeqModel
    O, ocfg, mcfg, W, batch = make("c4_bimodal_uni", use_dropout=True, sampling_probability=0.3)
    ref = O.train_step(W, None, ocfg, batch)
    db = Batch.from_numpy(batch)
    losses = []
    for off in (0, 1 << 24, 2 << 24):
        m = Seq2SeqModel(mcfg, weights=W)
        m.seed_offset = off
        m.forward_train(db)
        torch.cuda.synchronize()
        losses.append(float(m.loss.item()))
    # offset 0 = the oracle's masks: the forward-only loss scalar is the sequence term + the AU term (L2 joins in apply_update)
    assert abs(losses[0] - (ref["seq_loss"] + ref["au_term"])) < 1e-4, (losses[0], ref["seq_loss"], ref["au_term"])
    assert len({round(x, 6) for x in losses}) == 3, losses
