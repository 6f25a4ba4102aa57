"""Exact one-layer evaluator with a derived error bound (TEST INFRASTRUCTURE ONLY -- see oracle/__init__.py).

The bf16 engine is compared layer by layer: every layer is fed with the engine's OWN stored input tensors ("teacher forcing")
and evaluated in float64.  What the engine may then differ by is float32 accumulation error plus one rounding to bf16, and
both have textbook bounds per element -- nothing here is measured on the code under test.

Per op, with inputs x (float64 value) and e_x (their bound; 0 where the tensor was forced):
    s = sum w*x + b (+ add)                         float64
    A = sum |w|*(|x| + e_x) + |b| (+ |add| + e_add)
    E = sum |w|*e_x (+ e_add)
    K = number of summed terms, bias and add included
    gamma = K*u / (1 - K*u),  u = 2^-23             a float32 sum of K terms in ANY order (Higham, Accuracy and Stability of
                                                    Numerical Algorithms, 2nd ed., eq. 3.5, (4.4)); twice the round-to-nearest unit roundoff, so
                                                    that it also holds for an adder that truncates
    d = E + gamma*A + K*2^-126                      the last term: flushed subnormals
    bound = d + 2^-8*(|s| + d) + 2^-133             where the tensor is rounded to bf16 (8 significant bits, nearest; 2^-133: the
                                                    spacing of bf16 subnormals); bound = d for the float32 logits
ReLU, max-pool, up-sampling and concat act on s; the bound passes through them (all are 1-Lipschitz; a pool takes the
window's maximum).  BatchNormalization in the engine's bf16 form: s = x*scale + shift, K = 2, E = |scale|*e_x.

The graphs are oracle/models.py's own functions (_fcn, _unet, _res_unet), walked with another context object."""
from collections import OrderedDict, namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from . import core, models

U_F32 = 2.0 ** -23          # see gamma above
U_F32_NEAREST = 2.0 ** -24  # round-to-nearest unit roundoff (what the oracle's own sums satisfy)
U_BF16 = 2.0 ** -8
TINY_F32 = 2.0 ** -126
TINY_BF16 = 2.0 ** -133

Layer = namedtuple("Layer", "s bound all_forced inputs")      # s, bound: float64 (H, W, C); inputs: names of the producing ops read
Report = namedtuple("Report", "count ratio worst")            # worst: [(layer, y, x, channel, error, bound)], largest error / bound first


class _T:
    """A tensor in flight: value, bound per element, whether every element is a forced (or exact) value, producing ops."""
    __slots__ = ("s", "e", "forced", "deps")

    def __init__(self, s, e, forced, deps):
        self.s, self.e, self.forced, self.deps = s, e, forced, frozenset(deps)


def _t4(a):
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))[None]


def _same(x4, k, stride):
    """TF SAME: pad_before = total // 2, the rest behind (k2: 0 / 1; k3 s2 on an even size: 0 / 1)."""
    pads = []
    for n in (x4.shape[3], x4.shape[2]):                      # F.pad: last dimension first
        _, before = core.same_pad(n, k, stride)
        total = max((-(-n // stride) - 1) * stride + k - n, 0)
        pads += [before, total - before]
    return F.pad(x4, pads)


class _Exact:
    """The interface oracle/models.py's graph functions use (models._Ctx), over _T."""

    def __init__(self, Wt, forced, u):
        self.W = models.to_bf16_weights(Wt)
        self.forced = forced
        self.u = float(u)
        self.nm = models._Namer()
        self.out = OrderedDict()

    # ---- value-preserving ops -------------------------------------------------------------------------------------------
    @staticmethod
    def pad32(x):
        s, pads = models._pad32(x.s)
        return _T(s, models._pad32(x.e)[0], x.forced, x.deps), pads

    @staticmethod
    def crop(x, pads):
        return _T(models._crop(x.s, pads), models._crop(x.e, pads), x.forced, x.deps)

    @staticmethod
    def up2(x):
        return _T(models._up2(x.s), models._up2(x.e), x.forced, x.deps)

    @staticmethod
    def cat(a, b):
        return _T(np.concatenate([a.s, b.s], -1), np.concatenate([a.e, b.e], -1), a.forced and b.forced, a.deps | b.deps)

    # ---- ops --------------------------------------------------------------------------------------------------------------
    def _emit(self, name, s, bound, ins):
        """Record the op's exact value and bound; hand its readers the engine's tensor where there is one."""
        self.out[name] = Layer(s, bound, all(t.forced for t in ins), tuple(sorted(frozenset().union(*[t.deps for t in ins]))))
        if name in self.forced:
            g = np.asarray(self.forced[name], np.float64)
            assert g.shape == s.shape, "%s: forced tensor %r, layer %r" % (name, g.shape, s.shape)
            return _T(g, np.zeros_like(g), True, (name,))
        return _T(s, bound, False, (name,))

    def _finish(self, name, s, A, E, K, relu, ins, rounded=True):
        gamma = K * self.u / (1.0 - K * self.u)
        d = E + gamma * A + K * TINY_F32
        if relu:
            s = np.maximum(s, 0.0)
        bound = d + U_BF16 * (np.abs(s) + d) + TINY_BF16 if rounded else d
        return self._emit(name, s, bound, ins)

    def _lin(self, x, w_oihw, b, fn, add=None, in_relu=False):
        """fn(x4, w4) -> y4: the linear map (a correlation or a transposed convolution), applied to values and to magnitudes."""
        xs = np.maximum(x.s, 0.0) if in_relu else x.s
        w = torch.from_numpy(np.ascontiguousarray(w_oihw, dtype=np.float64))
        hwc = lambda y4: y4[0].permute(1, 2, 0).contiguous().numpy()
        b = np.asarray(b, np.float64)
        s = hwc(fn(_t4(xs), w)) + b
        A = hwc(fn(_t4(np.abs(xs) + x.e), w.abs())) + np.abs(b)
        E = hwc(fn(_t4(x.e), w.abs())) if x.e.any() else np.zeros_like(s)
        ins = [x]
        if add is not None:
            s, A, E = s + add.s, A + np.abs(add.s) + add.e, E + add.e
            ins.append(add)
        return s, A, E, ins

    def conv(self, x, relu=False, stride=1, name=None, add=None, in_relu=False, keep=None):
        name = name or self.nm("conv2d")
        Kw = self.W[name + "/kernel"]                                   # (kh, kw, Cin, Cout)
        k = Kw.shape[0]
        fn = lambda x4, w4: F.conv2d(_same(x4, k, stride), w4, stride=stride)
        s, A, E, ins = self._lin(x, Kw.transpose(3, 2, 0, 1), self.W[name + "/bias"], fn, add=add, in_relu=in_relu)
        K = k * k * Kw.shape[2] + 1 + (add is not None)
        return self._finish(keep or name, s, A, E, K, relu, ins, rounded=name != "logits")

    def tconv5(self, x, relu=False):
        """Conv2DTranspose k5 s1 SAME == correlation with the flipped, channel-swapped kernel."""
        name = self.nm("conv2d_transpose")
        Kw = self.W[name + "/kernel"]                                   # (5, 5, Cout, Cin)
        w = np.ascontiguousarray(Kw[::-1, ::-1]).transpose(2, 3, 0, 1)   # -> (Cout, Cin, 5, 5)
        fn = lambda x4, w4: F.conv2d(_same(x4, 5, 1), w4)
        s, A, E, ins = self._lin(x, w, self.W[name + "/bias"], fn)
        return self._finish(name, s, A, E, 25 * Kw.shape[3] + 1, relu, ins)

    def deconv2(self, x, relu=False):
        """Conv2DTranspose k2 s2: out[2y + a, 2x + b] = sum_ci x[y, x, ci] * K[a, b, co, ci] -- one tap per output pixel."""
        name = self.nm("conv2d_transpose")
        Kw = self.W[name + "/kernel"]                                   # (2, 2, Cout, Cin)
        fn = lambda x4, w4: F.conv_transpose2d(x4, w4, stride=2)
        s, A, E, ins = self._lin(x, Kw.transpose(3, 2, 0, 1), self.W[name + "/bias"], fn)   # (Cin, Cout, 2, 2)
        return self._finish(name, s, A, E, Kw.shape[3] + 1, relu, ins)

    def bn(self, x, name, relu=False):
        g, b = self.W[name + "/gamma"], self.W[name + "/beta"]
        m, v = self.W[name + "/moving_mean"], self.W[name + "/moving_variance"]
        scale32 = (g / np.sqrt(v + models.BN_EPS)).astype(np.float32)   # the float32 scale / shift the engine is given
        shift = (b - m * scale32).astype(np.float32).astype(np.float64)
        scale = scale32.astype(np.float64)
        s = x.s * scale + shift
        A = np.abs(scale) * (np.abs(x.s) + x.e) + np.abs(shift)
        return self._finish(name, s, A, np.abs(scale) * x.e, 2, relu, [x])

    def pool(self, x):
        """MaxPooling2D 2x2 in float64: exact on forced values, the window's largest bound otherwise."""
        name = self.nm("max_pooling2d")
        H, W, C = x.s.shape
        win = lambda a: a.reshape(H // 2, 2, W // 2, 2, C).max(axis=(1, 3))
        y = self._emit(name, win(x.s), win(x.e), [x])
        if not y.forced:
            y.forced = x.forced          # the pool of forced tensors is exact: as good as forced
        return y


def input_canvas(image_u8):
    """The network input on the pad-to-32 canvas, (Hp, Wp, C) float32 holding bf16 values: what the engine's "input" tensor is."""
    img = np.asarray(image_u8)
    x = core.round_bf16(core.preprocess(img))
    return models._pad32(x[..., None] if img.ndim == 2 else x)[0]


def evaluate(arch, Wt, image_u8, forced, u=U_F32):
    """-> OrderedDict op name -> Layer(s, bound, all_forced, inputs), in graph order; the last one is "logits" (cropped).
    Wt: the weight table (kernels are rounded to bf16 here, as to_bf16_weights does; biases stay float32).
    forced: {layer name: the engine's tensor, float32 holding bf16 values, on the canvas}; "input" may be among them."""
    img = np.asarray(image_u8)
    assert img.dtype == np.uint8 and img.ndim in (2, 3)
    c = _Exact(Wt, forced, u)
    H, W = img.shape[:2]
    x = input_canvas(img) if "input" not in forced else np.asarray(forced["input"])
    x = np.asarray(x[:H, :W], np.float64)                     # (the graph pads again)
    x = _T(x, np.zeros_like(x), True, ("input",))
    if arch in ("fcn_skip", "fcn"):
        models._fcn(c, x, arch == "fcn_skip")
    elif arch == "unet":
        models._unet(c, x)
    elif arch == "res_unet":
        models._res_unet(c, x, bn="batch_normalization/gamma" in Wt)
    else:
        raise ValueError(arch)
    return c.out


def check(engine_tensor, s, bound, layer="", n_worst=5):
    """Elements with |g - s| > bound (a NaN counts) -> Report(count, max error / bound, worst offenders)."""
    g = np.asarray(engine_tensor, np.float64)
    assert g.shape == s.shape, "%s: engine tensor %r, exact layer %r" % (layer, g.shape, s.shape)
    err = np.abs(g - s)
    bad = ~(err <= bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bad & ~np.isfinite(err), np.inf, np.where(err == 0, 0.0, err / bound))   # (bound 0: an exact op)
    worst = []
    if bad.any():
        idx = np.argwhere(bad)
        order = np.argsort(-ratio[bad], kind="stable")[:n_worst]
        worst = [(layer, int(y), int(x), int(ch), float(err[y, x, ch]), float(bound[y, x, ch])) for y, x, ch in idx[order]]
    return Report(int(bad.sum()), float(ratio.max()) if ratio.size else 0.0, worst)


def check_labels(pred, s, bound):
    """The label rule on the exact forced logits: pred must be argmax(s) wherever the top-2 margin of s exceeds the sum of the
    two bounds at that pixel; elsewhere either of the two is accepted.  -> (wrong pixels, excused share of the page)."""
    order = np.argsort(-s, axis=-1, kind="stable")
    i1, i2 = order[..., 0], order[..., 1]
    take = lambda a, i: np.take_along_axis(a, i[..., None], -1)[..., 0]
    excused = ~(take(s, i1) - take(s, i2) > take(bound, i1) + take(bound, i2))
    ok = (pred == i1) | (excused & (pred == i2))
    return int((~ok).sum()), float(excused.mean())
