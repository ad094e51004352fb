"""Independent fp64 restatement of the reference's spatio-temporal front-end `video.conv3d_cnn` (avsr/video.py:34-46, :92-105,
:198-222) on torch.nn.functional.conv3d, for the tests of video_processing='3dconv_cnn'.

  flow = inputs*2 - 1; conv3d(f0, (1,3,3)) -> BN-ReLU; residual_block_3d((3,3,3), stride 1, skip_bn, identity shortcut);
  per further filter count: BN-ReLU, projection conv3d (1,1,1)/(1,2,2) of the un-normalised input, conv3d (3,3,3)/(1,2,2), BN-ReLU,
  conv3d (3,3,3), + shortcut; conv3d(dense, [1, H', W'], VALID, relu) squeezed to [B, T, dense].
No biases (conv3d_wrapper: use_bias=False).  TF SAME padding on every axis, the odd pixel after.  Batch norms: epsilon 1e-5, momentum
0.98, TF 1.13's non-fused path on rank-5 maps (avsr_oracle.batch_norm(..., fused=False): biased moving variance).  The reference's
final conv3d passes strides=(1, 1); it is restated with (1, 1, 1)."""
import math

import numpy as np
import torch

from oracle import avsr_oracle as O

PREFIX = "video/cnn/"


def same_pad(n, k, s):
    """TF 'SAME' along one axis: (out, pad before, pad after)."""
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return out, total // 2, total - total // 2


def layout(hw, filters, dense):
    """[(kind, name, args)] in the order the reference's graph creates the layers."""
    H, W, C = hw
    f = list(filters)
    L = [("conv", "layer0", dict(k=(1, 3, 3), s=1, cin=C, cout=f[0], src="in", dst="a0")),
         ("bnrelu", "layer0_bn", dict(c=f[0], src="a0", dst="b0")),
         ("conv", "res_block_0_conv1", dict(k=(3, 3, 3), s=1, cin=f[0], cout=f[0], src="b0", dst="r0a")),
         ("bnrelu", "res_block_0_second_bn", dict(c=f[0], src="r0a", dst="r0b")),
         ("conv", "res_block_0_conv2", dict(k=(3, 3, 3), s=1, cin=f[0], cout=f[0], src="r0b", dst="r0c")),
         ("add", "res_block_0", dict(a="r0c", b="b0", dst="x0"))]
    prev, cin = "x0", f[0]
    for i, c in enumerate(f[1:], start=1):
        n = "res_block_%d" % i
        L += [("bnrelu", n + "_first_bn", dict(c=cin, src=prev, dst=n + "_p")),
              ("conv", n + "_shortcut", dict(k=(1, 1, 1), s=2, cin=cin, cout=c, src=prev, dst=n + "_s")),
              ("conv", n + "_conv1", dict(k=(3, 3, 3), s=2, cin=cin, cout=c, src=n + "_p", dst=n + "_a")),
              ("bnrelu", n + "_second_bn", dict(c=c, src=n + "_a", dst=n + "_b")),
              ("conv", n + "_conv2", dict(k=(3, 3, 3), s=1, cin=c, cout=c, src=n + "_b", dst=n + "_c")),
              ("add", n, dict(a=n + "_c", b=n + "_s", dst="x%d" % i))]
        prev, cin = "x%d" % i, c
        H, W = same_pad(H, 3, 2)[0], same_pad(W, 3, 2)[0]
    L.append(("final", "flatten", dict(k=(1, H, W), cin=cin, cout=dense, src=prev, dst="out")))
    return L


def param_shapes(hw, filters, dense):
    out = []
    for kind, name, a in layout(hw, filters, dense):
        if kind in ("conv", "final"):
            out.append((name + "/kernel", tuple(a["k"]) + (a["cin"], a["cout"])))
        elif kind == "bnrelu":
            out += [(name + "/" + v, (a["c"],)) for v in ("gamma", "beta", "moving_mean", "moving_variance")]
    return out


def tf_names(hw, filters, dense):
    """TF's auto-generated layer names in creation order: conv3d, conv3d_1, ...; batch_normalization, batch_normalization_1, ..."""
    out, nc, nb = {}, 0, 0
    for kind, name, _a in layout(hw, filters, dense):
        if kind in ("conv", "final"):
            out[name + "/kernel"] = "conv3d" + ("_%d" % nc if nc else "") + "/kernel"
            nc += 1
        elif kind == "bnrelu":
            for v in ("gamma", "beta", "moving_mean", "moving_variance"):
                out[name + "/" + v] = "batch_normalization" + ("_%d" % nb if nb else "") + "/" + v
            nb += 1
    return out


def init_params(hw, filters, dense, seed=5):
    """variance_scaling_initializer(2.0, fan_in) kernels (fan_in = kt*kh*kw*cin), unit gamma, zero beta, zero / unit moving stats."""
    rng = np.random.default_rng(seed)
    P = {}
    for name, shape in param_shapes(hw, filters, dense):
        if name.endswith("/kernel"):
            std = math.sqrt(2.0 / int(np.prod(shape[:-1]))) / 0.87962566103423978
            x = rng.standard_normal(shape)
            bad = np.abs(x) > 2.0
            while bad.any():
                x[bad] = rng.standard_normal(int(bad.sum()))
                bad = np.abs(x) > 2.0
            P[PREFIX + name] = (x * std).astype(np.float32)
        else:
            v = 1.0 if name.endswith(("gamma", "moving_variance")) else 0.0
            P[PREFIX + name] = np.full(shape, v, np.float32)
    return P


def conv3d_same(x, w, s, valid=False):
    """x [B, T, H, W, C]; w [kt, kh, kw, cin, cout]; strides (1, s, s); TF SAME (or VALID) padding."""
    F = torch.nn.functional
    kt, kh, kw = w.shape[:3]
    xt = x.permute(0, 4, 1, 2, 3)
    if not valid:
        _, f0, f1 = same_pad(x.shape[1], kt, 1)
        _, t0, t1 = same_pad(x.shape[2], kh, s)
        _, l0, l1 = same_pad(x.shape[3], kw, s)
        xt = F.pad(xt, (l0, l1, t0, t1, f0, f1))
    return F.conv3d(xt, w.permute(4, 3, 0, 1, 2), stride=(1, s, s)).permute(0, 2, 3, 4, 1)


def forward(P, hw, filters, dense, frames, training, updates, masks=None):
    """frames [B, T, H, W, C] -> [B, T, dense]; `updates` receives the moving statistics (non-fused rule).
    masks {layer name: 0/1 tensor}: use these ReLU masks instead of the restatement's own signs (the gradient of a ReLU whose input lies
    within rounding of zero differs between fp32 and fp64 by that element's whole contribution; with the masks an implementation took,
    what remains to compare is arithmetic)."""
    maps = {"in": frames * 2 - 1}
    for kind, name, a in layout(hw, filters, dense):
        pre = PREFIX + name
        if kind == "conv":
            maps[a["dst"]] = conv3d_same(maps[a["src"]], P[pre + "/kernel"], a["s"])
        elif kind == "bnrelu":
            y = O.batch_norm(maps[a["src"]], P, pre, training, updates, eps=1e-5, momentum=0.98, fused=False)
            maps[a["dst"]] = y * masks[name] if masks else torch.relu(O._note_relu(y))
        elif kind == "add":
            maps[a["dst"]] = maps[a["a"]] + maps[a["b"]]
        else:
            y = conv3d_same(maps[a["src"]], P[pre + "/kernel"], 1, valid=True)
            y = y * masks[name].reshape(y.shape) if masks else torch.relu(O._note_relu(y))
            maps["out"] = y.reshape(y.shape[0], y.shape[1], -1)
    return maps["out"]


def patch_oracle(monkeypatch, cfg, T, masks=None):
    """Route the oracle's lip-CNN front-end through this restatement: its cnn_forward sees [B*T, H, W, C] frames.  masks: see forward
    (training graphs only)."""
    def cnn_forward(P, ocfg, frames, training, updates):
        BT = frames.shape[0]
        x = frames.reshape((BT // T, T) + tuple(frames.shape[1:]))
        return forward(P, ocfg.video_hw, ocfg.cnn_filters, ocfg.cnn_dense_units, x, training, updates,
                       masks if training else None).reshape(BT, -1)
    monkeypatch.setattr(O, "cnn_forward", cnn_forward)


def swap_params(W, hw, filters, dense, seed=5):
    """Oracle parameters with the 2-D front-end's video/cnn/ entries replaced by the 3-D ones."""
    out = {k: v for k, v in W.items() if not k.startswith(PREFIX)}
    out.update(init_params(hw, filters, dense, seed))
    return out
