"""Spatio-temporal lip front-end: `video.conv3d_cnn` (avsr/video.py:198-222, selected at :241-243) on the HIP engine.

[B, T, H, W, C] lip crops, the whole padded batch as ONE 5-D map (no folding of frames into the batch):
flow = inputs*2 - 1 -> conv3d (1,3,3) -> BN-ReLU -> residual_block_3d (3,3,3), identity shortcut, no leading BN -> one block per
further filter count (BN-ReLU, 1x1x1 / (1,2,2) projection shortcut on the un-normalised input, conv (3,3,3)/(1,2,2), BN-ReLU,
conv (3,3,3), add) -> conv3d [1, H', W'] VALID + ReLU -> [B, T, cnn_dense_units].  Every conv3d has use_bias=False, a variance-scaling
(2, fan_in) kernel and l2(0.001) (video.py:34-46); BN: epsilon 1e-5, momentum 0.98 (video.py:4-14) on rank-5 maps, i.e. TF 1.13's
NON-fused batch norm (biased moving variance).  SAME padding per axis with the odd pixel after; in time (stride 1, kernel 3) one zero
frame before frame 0 and one after frame T_max - 1 of the padded batch, none at an utterance's own length: padding frames (-1 after
the affine) take part, as in the reference.  The reference's final conv3d passes strides=(1, 1); it is built here with (1, 1, 1)
(INTEGRATION.md section 8).

The convolutions run on the implicit-GEMM MFMA kernels of csrc/conv3d.hip (avsr_conv3d_fwd / _bwd_data / _bwd_weight).  Fusions: the
producing convolution's epilogue adds the residual and emits the batch-norm partial sums of what it wrote; batch norms are applied by
their consumers' loaders (forward and weight gradient), so no normalised map is written; layer 0's `*2-1` is the same loader transform
without the ReLU.  The batch-norm backward is avsr_bn_bwd_stage1 / avsr_bn_bwd_finalize / avsr_bn_bwd_apply.  The final [1, H', W']
VALID convolution is per frame: one GEMM over the [B*T, H'*W'*C] rows, no bias.  This file only owns buffers and the op order."""
import torch

from . import ops
from .cnn import resnet_layout, resnet_param_shapes, same_pad


def layout(hw, filters, dense):
    """Op list of conv3d_cnn in graph order.  ('conv', name, src, dst, (kt, kh, kw), stride, cin, cout) | ('bnrelu', name, src, dst, c) |
    ('add', name, a, b, dst) | ('flatten', name, src, dst, kh, kw, cin, cout);  shapes[name] = (H, W, C) of every map (per frame)."""
    return resnet_layout(hw, filters, dense, (1, 3, 3), (3, 3, 3), (1, 1, 1))


def param_shapes(hw, filters, dense):
    """[(name, tf_shape, role)] in graph order; role: conv_kernel | gamma | beta | moving_mean | moving_variance (no biases)."""
    return resnet_param_shapes(layout(hw, filters, dense)[0], bias=False)


def tf_names(hw, filters, dense):
    """{engine name: TF variable name}: tf.layers.conv3d / batch_normalization take the auto-generated names conv3d, conv3d_1, ... and
    batch_normalization, batch_normalization_1, ... in the order the graph creates them (video.py:92-105: a block's leading BN, then its
    projection shortcut, conv1, second BN, conv2)."""
    out, nc, nb = {}, 0, 0
    for name, _shape, role in param_shapes(hw, filters, dense):
        layer, var = name.rsplit("/", 1)
        if role == "conv_kernel":
            out[name] = "conv3d%s/kernel" % ("_%d" % nc if nc else "")
            nc += 1
        else:
            out[name] = "batch_normalization%s/%s" % ("_%d" % nb if nb else "", var)
            if var == "moving_variance":
                nb += 1
    return out


class LipCNN3D:
    BN_EPS, BN_MOMENTUM, L2 = 1e-5, 0.98, 1e-3

    def __init__(self, model, B, T, prefix="video/cnn/", grads=True):
        cfg = model.cfg
        self.m, self.B, self.T, self.N, self.pre = model, B, T, B * T, prefix
        self.ops, self.shapes = layout(cfg.video_hw, cfg.cnn_filters, cfg.cnn_dense_units)
        dev = model.dev
        z = lambda *s: torch.zeros(*s, device=dev)
        N = self.N
        self.geo = {}
        for op in self.ops:
            if op[0] == "conv":
                _, name, src, dst, k, s, cin, cout = op
                h, w, _ = self.shapes[src]
                ho, pt = same_pad(h, k[1], s)
                wo, pl = same_pad(w, k[2], s)
                self.geo[name] = (B, T, h, w, cin, cout, k, s, ((k[0] - 1) // 2, pt, pl), ho, wo)
                if not ops.conv3d_supported(ops.conv3d_desc(*self.geo[name])):
                    raise NotImplementedError("3dconv_cnn: layer %s (%d -> %d channels) is outside the conv3d kernels' budget" % (name, cin, cout))
        # the second convolution of every residual block adds the shortcut in its epilogue (the add's operand map never exists)
        by_dst = {op[3]: op for op in self.ops if op[0] == "conv"}
        self.fuse_add = {}
        for op in self.ops:
            if op[0] == "add":
                self.fuse_add[by_dst[op[2]][1]] = (op[3], op[4])
        bn_src = {op[2] for op in self.ops if op[0] == "bnrelu"}
        self.bn, self.stat_buf, self.bnb_part, self.bnb_k = {}, {}, {}, {}
        for op in self.ops:
            if op[0] == "bnrelu":
                c = op[4]
                self.bn[op[1]] = (z(c), z(c), z(c), z(c))          # batch mean, inverse std; scale, shift of the loader transform
                self.stat_buf[op[2]] = z(512 * 2 * c)
                self.bnb_part[op[1]], self.bnb_k[op[1]] = z(512 * 2 * c), z(3 * c)
        self.bn_src = bn_src
        # stored maps: pre-normalisation conv outputs, shortcut outputs and block outputs (never a normalised map)
        stored = {"a0", "r0a", "x0"}
        for i in range(1, len(cfg.cnn_filters)):
            stored |= {"res_block_%d_s" % i, "res_block_%d_a" % i, "x%d" % i}
        self.maps, self.gmaps = {}, {}
        big = 0
        for name in stored:
            h, w, c = self.shapes[name]
            self.maps[name] = z(N, h, w, c)
            big = max(big, N * h * w * c)
            if grads and not name.endswith("_s"):
                self.gmaps[name] = z(N, h, w, c)
        # gradient maps only in a workspace that runs backward passes (a decoding workspace never does)
        self.has_grads = grads
        if grads:
            for i in range(1, len(cfg.cnn_filters)):             # the shortcut's gradient is its block output's (identity add)
                self.gmaps["res_block_%d_s" % i] = self.gmaps["x%d" % i]
        self.gbn = z(big) if grads else None                     # gradient of a batch norm's output (transient, reused)
        self.pre_act = z(N, cfg.cnn_dense_units)
        self.maps["out"] = z(N, cfg.cnn_dense_units)
        Cin = self.shapes["in"][2]
        self.in_tf = (torch.full((Cin,), 2.0, device=dev), torch.full((Cin,), -1.0, device=dev))   # flow = inputs * 2 - 1
        need = max(ops.conv3d_wgrad_scratch_floats(ops.conv3d_desc(*g)) for g in self.geo.values()) if grads else 4
        shared = getattr(model, "_cnn3d_wg_scratch", None)       # one buffer per model: weight gradients run one after another
        if shared is None or shared.numel() < need:
            shared = model._cnn3d_wg_scratch = torch.empty(max(need, 4), device=dev)
        self.wg_scratch = shared
        self.lazy = {}

    def _p(self, n):
        return self.m.P[self.pre + n]

    def _g(self, n):
        return self.m.Gr[self.pre + n]

    def _pv(self, n):
        return self.m._pp(self.pre + n)

    def _src(self, name):
        """(map, loader transform | None, relu): the crops through `*2-1`, a lazily normalised map through its BN-ReLU, or a stored map."""
        if name == "in":
            return self.maps["in"], self.in_tf, 0
        lz = self.lazy.get(name)
        if lz:
            return self.maps[lz[0]], (lz[1], lz[2]), 1
        return self.maps[name], None, 1

    def _desc(self, name, src):
        x, tf, relu = self._src(src)
        return ops.conv3d_desc(*self.geo[name], tf=tf, relu=relu), x

    def forward(self, frames, training):
        m, N = self.m, self.N
        H, W, C = self.shapes["in"]
        assert frames.shape == (N, H, W, C) and frames.is_contiguous() and frames.dtype == torch.float32
        if training and getattr(m, "cnn_bn_sync", None) is not None:
            raise NotImplementedError("sync_cnn_bn is not built for video_processing='3dconv_cnn' (per-rank batch norms only)")
        self.maps["in"] = frames
        self.lazy = {}
        rows = {}
        for op in self.ops:
            kind = op[0]
            if kind == "conv":
                name, src, dst = op[1], op[2], op[3]
                d, x = self._desc(name, src)
                res, res_tf, out = None, None, dst
                if name in self.fuse_add:
                    sc_name, out = self.fuse_add[name]
                    res, tf, _relu = self._src(sc_name)
                    res_tf = tf
                stats = self.stat_buf[out] if (training and out in self.bn_src) else None
                kw_ = self._p(name + "/kernel")
                rows[out] = ops.conv3d_fwd(d, x, kw_.t[kw_.off:], self.maps[out], res=res, res_tf=res_tf, stats=stats)
            elif kind == "bnrelu":
                _, name, src, dst, c = op
                h, w, _ = self.shapes[src]
                mean, invstd, scale, shift = self.bn[name]
                if training:
                    # seq2seq.py:241-250: the moving averages only move with the train op under batch_normalisation=True
                    upd = m.cfg.batch_normalisation
                    ops.conv3d_bn_finalize(self.stat_buf[src], rows[src], c, N * h * w, self.BN_EPS, self.BN_MOMENTUM, mean, invstd,
                                           m._sp(self.pre + name + "/moving_mean") if upd else None,
                                           m._sp(self.pre + name + "/moving_variance") if upd else None,
                                           self._pv(name + "/gamma"), self._pv(name + "/beta"), scale, shift)
                else:
                    ops.bn_eval_affine(self._pv(name + "/gamma"), self._pv(name + "/beta"), m._sp(self.pre + name + "/moving_mean"),
                                       m._sp(self.pre + name + "/moving_variance"), self.BN_EPS, scale, shift, c)
                self.lazy[dst] = (src, scale, shift)
            elif kind == "add":
                continue                                         # done by the second convolution's epilogue
            else:
                _, name, src, dst, kh, kw, cin, cout = op
                K = kh * kw * cin
                ops.gemm(ops.mat(self.maps[src], K), self._p(name + "/kernel").mat(cout), ops.mat(self.pre_act, cout), N, cout, K)
                ops.relu(self.pre_act, self.maps[dst], N * cout)
        return self.maps["out"].view(N, -1)

    def _wgrad(self, name, src, dy):
        d, x = self._desc(name, src)
        gk = self._g(name + "/kernel")
        ops.conv3d_bwd_weight(d, x, dy, gk.t[gk.off:], self.wg_scratch, beta=1.0)

    def _dgrad(self, name, dy, dx, beta):
        kw_ = self._p(name + "/kernel")
        ops.conv3d_bwd_data(ops.conv3d_desc(*self.geo[name]), dy, kw_.t[kw_.off:], dx, beta=beta)

    def _bn_bwd(self, name, src, gy, out, beta=0.0):
        """gy = gradient of relu(bn(src)) (overwritten by dz); out (+)= the gradient wrt src."""
        c = self.shapes[src][2]
        h, w, _ = self.shapes[src]
        rows = self.N * h * w
        mean, invstd, scale, shift = self.bn[name]
        x = self.maps[src]
        n = ops.bn_bwd_stage1(gy, x, gy, rows, c, self.bnb_part[name], scale=scale, shift=shift)
        gg, gb = self._g(name + "/gamma"), self._g(name + "/beta")
        ops.bn_bwd_finalize(self.bnb_part[name], n, c, rows, mean, invstd, self._pv(name + "/gamma"), gg.t[gg.off:gg.off + c],
                            gb.t[gb.off:gb.off + c], self.bnb_k[name], grad_beta=0.0)
        ops.bn_bwd_apply(gy, x, self.bnb_k[name], out, rows, c, beta=beta)

    def _gbn(self, name):
        h, w, c = self.shapes[name]
        return self.gbn[:self.N * h * w * c]

    def backward(self, dfeat):
        """dfeat [N, cnn_dense_units]: gradient of the loss wrt the front-end output.  Accumulates into the model's gradient buffer."""
        m, N = self.m, self.N
        assert self.has_grads, "LipCNN3D.backward on a decoding workspace (no gradient maps)"
        nb = len(m.cfg.cnn_filters)
        fl = self.ops[-1]
        _, name, src, dst, kh, kw, cin, cout = fl
        K = kh * kw * cin
        ops.relu_bwd(self.maps["out"], dfeat, self.pre_act, N * cout)     # pre_act now holds d(pre-activation)
        m._gemm_tn(ops.mat(self.maps[src], K), ops.mat(self.pre_act, cout), self._g(name + "/kernel").mat(cout), K, cout, N)
        ops.gemm(ops.mat(self.pre_act, cout), self._p(name + "/kernel").mat(cout), ops.mat(self.gmaps[src], K), N, K, cout, trans_b=1)
        for i in reversed(range(1, nb)):
            n, prev, gx = "res_block_%d" % i, "x%d" % (i - 1), self.gmaps["x%d" % i]
            a = n + "_a"
            self._wgrad(n + "_conv2", n + "_b", gx)
            gb = self._gbn(a)
            self._dgrad(n + "_conv2", gx, gb, 0.0)
            self._bn_bwd(n + "_second_bn", a, gb, self.gmaps[a])
            self._wgrad(n + "_conv1", n + "_p", self.gmaps[a])
            gp = self._gbn(prev)
            self._dgrad(n + "_conv1", self.gmaps[a], gp, 0.0)
            self._bn_bwd(n + "_first_bn", prev, gp, self.gmaps[prev])
            self._wgrad(n + "_shortcut", prev, gx)
            self._dgrad(n + "_shortcut", gx, self.gmaps[prev], 1.0)
        gx0 = self.gmaps["x0"]
        self._wgrad("res_block_0_conv2", "r0b", gx0)
        gb = self._gbn("r0a")
        self._dgrad("res_block_0_conv2", gx0, gb, 0.0)
        self._bn_bwd("res_block_0_second_bn", "r0a", gb, self.gmaps["r0a"])
        self._wgrad("res_block_0_conv1", "b0", self.gmaps["r0a"])
        gb = self._gbn("a0")
        self._dgrad("res_block_0_conv1", self.gmaps["r0a"], gb, 0.0)
        ops.add(gb, gx0, gb, gb.numel())                             # the identity shortcut: b0 also feeds the block's add
        self._bn_bwd("layer0_bn", "a0", gb, self.gmaps["a0"])
        self._wgrad("layer0", "in", self.gmaps["a0"])
