"""The image stem's kernels (csrc/qa_conv.hip, the window GEMMs qa_conv_nhwc_* of csrc/qa_gemm.hip) against tests/depth_stem_ref.py, a float64
statement of the same operations, at the edges the friendly shapes of tests/test_depth_stem.py never reach: more than 1,024 stem-backward items (the
grid-stride loop of a BYOL or DAgger batch), exact pool ties on clipped images, the widest / narrowest / odd image widths, one-row last bands, bands
of fewer than 8 pooled pixels, alpha != 1, every window-GEMM tile configuration at ragged channel and pixel counts, 257 output pixels, a 1 x 2 kernel,
activations 0 and 2, a missing bias, the weight gradient's split plan at its cap of 192.

CPU: the oracle's twins (qo_*) against the reference on every case; that the comparisons have teeth; what the twins refuse.
-m gpu: the same cases against the qa_* entries, called through the C ABI on raw pointers.  Every output and every scratch buffer is allocated at
exactly the size the ABI reports, between guard regions of 4 KiB filled with a quiet NaN's bit pattern that must come back bit-identical (on the CPU
too).  Every comparison uses the bound the reference carries, and every reduction is also run on small-integer operands on which the result must be
bit-equal to float64 (depth_stem_ref's docstring states both); there is no tolerance literal in this file.

Largest err / bound per group (bound = the carried worst-case bound, so ratios far below 1 are expected; `pytest -s` prints them as
"MEASURED worst err/bound so far, <who> <group>"):

    group                   MI355X          CPU twin
    stem forward            0.101           0.101
    stem backward           0.162           0.162
    pad                     0 (bit-equal)   0 (bit-equal)
    conv forward            0.072           0.064
    conv backward-input     0.029           0.021
    conv backward-weight    0.006           0.000

(The two largest are one rounding of an exact result against the (K + 2) u bound at K = 1: a single pooled pixel, and a negative ELU entry of the
exact pass.)
"""
import ctypes as C
import functools

import numpy as np
import pytest

from quadrupedal_agility_amd import _capi
from tests import depth_stem_ref as ref
from tests.oracle_lib import load_oracle

SENTINEL = 0x7FC5A5A5                       # a quiet NaN's bits: no arithmetic produces it, any store over it shows
GUARD_WORDS = 1024                          # 4 KiB before and after every exactly-sized buffer
E_ARG = -1                                  # QA_E_ARG
ALPHAS = (0.7, 1.0)
ALPHA = 0.7                                 # where one value is run


# ------------------------------------------------------------------------------------------------------------------------ the two sides of the ABI
class Guarded:
    """`nbytes` (a multiple of 4) between two guard regions, everything holding the sentinel"""

    def __init__(self, be, nbytes):
        assert nbytes > 0 and nbytes % 4 == 0
        self.be, self.words = be, nbytes // 4
        self.raw = be.alloc(self.words + 2 * GUARD_WORDS)
        self.ptr = C.c_void_p(be.addr(self.raw) + 4 * GUARD_WORDS)

    def read(self, dtype, shape, what):
        """the interior as a host array, after checking both guards"""
        h = self.be.host(self.raw)
        assert (h[:GUARD_WORDS] == SENTINEL).all(), f"{self.be.who}: {what}: written before its first byte"
        assert (h[GUARD_WORDS + self.words:] == SENTINEL).all(), f"{self.be.who}: {what}: written beyond its reported size"
        return h[GUARD_WORDS:GUARD_WORDS + self.words].view(dtype).reshape(shape).copy()


class Twin:
    who, prefix = "twin", "qo_"

    def __init__(self):
        self.lib = load_oracle()

    def alloc(self, words):
        return np.full(words, SENTINEL, np.int32)

    def addr(self, raw):
        return raw.ctypes.data

    def host(self, raw):
        return raw

    def put(self, a):
        a = np.ascontiguousarray(a)
        return a, C.c_void_p(a.ctypes.data)

    def call(self, name, *args):
        return getattr(self.lib, self.prefix + name)(*args, None)

    def size(self, name, *args):
        return getattr(self.lib, self.prefix + name)(*args)


class Hip:
    who, prefix = "hip", "qa_"

    def __init__(self):
        import torch
        self.torch, self.lib = torch, _capi.load_library()
        self.dev = torch.device("cuda", torch.cuda.current_device())

    def alloc(self, words):
        return self.torch.full((words,), SENTINEL, dtype=self.torch.int32, device=self.dev)

    def addr(self, raw):
        return raw.data_ptr()

    def host(self, raw):
        self.torch.cuda.synchronize()
        return raw.cpu().numpy()

    def put(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        return t, C.c_void_p(t.data_ptr())

    def call(self, name, *args):
        rc = getattr(self.lib, self.prefix + name)(*args, _capi.stream(self.dev))
        self.torch.cuda.synchronize()
        return rc

    def size(self, name, *args):
        return getattr(self.lib, self.prefix + name)(*args)


@functools.lru_cache(None)
def backend(who):
    return Twin() if who == "twin" else Hip()


# ------------------------------------------------------------------------------------------------------------------------ judging
_worst = {}


def _record(who, group, ratio):
    key = f"{who} {group}"
    _worst[key] = max(_worst.get(key, 0.0), ratio)
    print("MEASURED worst err/bound so far,", key, "= %.3f" % _worst[key])


def within(who, tag, got, res):
    """every element within the carried bound of the float64 value (a bound of zero: equal; a NaN is within nothing) -> the largest err / bound"""
    got = np.asarray(got, np.float64)
    err, bound = np.abs(got - res.val), np.broadcast_to(res.err, res.val.shape)
    assert np.isfinite(bound).all()
    ok = err <= bound
    pos = bound > 0
    ratio = float(np.nanmax(err[pos] / bound[pos])) if pos.any() else 0.0
    worst = int(np.nanargmax(np.where(np.isnan(err), np.inf, err / np.where(pos, bound, 1.0))))
    print("MEASURED", who, tag, "| max_err=%.3e bound_there=%.3e err/bound=%.3f" % (err.flat[worst], bound.flat[worst], ratio))
    assert ok.all(), f"{who}: {tag}: {int((~ok).sum())} of {ok.size} outside the bound, worst err {err.flat[worst]:.3e} against {bound.flat[worst]:.3e}"
    return ratio


def bit_equal(who, tag, got, val, where=None):
    """fp32 `got` against the float64 `val` of an exact pass, bit for bit (where `where`)"""
    g, w = np.asarray(got, np.float32).view(np.int32), ref.exact_bits(val)
    bad = (g != w) if where is None else ((g != w) & where)
    assert not bad.any(), f"{who}: {tag}: {int(bad.sum())} of {bad.size} differ from the exact value, first at {np.argwhere(bad)[0].tolist()}"


# ------------------------------------------------------------------------------------------------------------------------ stem forward
STEM_SHAPES = [(1, 6, 6), (2, 6, 126), (2, 23, 7), (2, 24, 125), (1, 40, 9), (1, 42, 10), (1, 6, 18), (3, 58, 87)]
SATURATED = (3, 58, 87)


@functools.lru_cache(None)
def stem_data(shape, kind):
    """real: seeded uniform images, continuous weights.  exact: images on the 1/8 grid in [-2, 2], weights and bias on the 1/16 grid in [-1/2, 1/2].
    saturated: an image clipped to its near and far constants, with whole constant columns and rows, under the exact pass's weights."""
    n, ih, iw = shape
    rng = np.random.default_rng([n, ih, iw, len(kind)])
    if kind == "real":
        img = rng.uniform(-0.5, 1.5, shape)
        w, b = rng.uniform(-0.2, 0.2, (32, 25)), rng.uniform(-0.1, 0.1, 32)
    else:
        img = rng.integers(-16, 17, shape) / 8
        w, b = rng.integers(-8, 9, (32, 25)) / 16, rng.integers(-8, 9, 32) / 16
        if kind == "saturated":
            near, far = 0.25, 2.0
            img = np.where(rng.random(shape) < 0.5, near, far)
            img[:, :, :iw * 2 // 5] = far                     # (nothing within range on the left)
            img[:, ih * 2 // 3:, :] = near                    # (the ground at the near clip)
            img[:, 5, :] = far
            img[:, :, iw - 7] = near
    return tuple(np.ascontiguousarray(a, np.float32) for a in (img, w, b))


@functools.lru_cache(None)
def stem_ref(shape, kind, alpha):
    return ref.stem_forward(*stem_data(shape, kind), alpha)


def run_stem_forward(be, shape, kind, alpha):
    n, ih, iw = shape
    ph, pw = ref.pooled_size(ih, iw)
    keep = [be.put(a) for a in stem_data(shape, kind)]
    y, am = Guarded(be, n * ph * pw * 32 * 4), Guarded(be, n * ph * pw * 32)
    assert be.call("depth_stem_forward", *[p for _, p in keep], y.ptr, am.ptr, n, ih, iw, alpha) == 0
    return y.read(np.float32, (n, ph, pw, 32), "stem y"), am.read(np.uint8, (n, ph, pw, 32), "stem argmax")


def undecided_share(r):
    return float((r.candidates.sum(3) > 1).mean())


def judge_stem_forward(who, tag, y, am, r, alpha, exact):
    assert (am <= 3).all(), f"{who}: {tag}: an argmax byte outside 0..3"
    if exact:
        assert np.array_equal(am, r.arg), f"{who}: {tag}: {int((am != r.arg).sum())} argmax bytes off the first-maximum rule"
        bit_equal(who, tag, y, np.where(r.pre.val >= 0, r.pre.val, 0.0), r.pre.val >= 0)
        return within(who, tag, y, ref.act_forward(1, alpha, r.pre.val, 0.0))
    assert undecided_share(r) <= ref.UNDECIDED_CAP, f"{tag}: the reference itself leaves {undecided_share(r):.5f} of the argmax undecided"
    picked = np.take_along_axis(r.candidates, am[:, :, :, None].astype(np.int64), 3)[:, :, :, 0]
    assert picked.all(), f"{who}: {tag}: {int((~picked).sum())} argmax bytes name a cell that float64 rules out"
    return within(who, tag, y, r.y)


def check_stem_forward(who, shape, alpha):
    be = backend(who)
    for kind in ("real", "exact"):
        y, am = run_stem_forward(be, shape, kind, alpha)
        _record(who, "stem forward", judge_stem_forward(who, f"stem forward {shape} {kind} alpha {alpha}", y, am, stem_ref(shape, kind, alpha), alpha, kind == "exact"))


def check_stem_saturated(who, alpha):
    r = stem_ref(SATURATED, "saturated", alpha)
    top = r.cells.max(3, keepdims=True)
    ties = ((r.cells == top).sum(3) > 1).mean()
    assert ties >= ref.SATURATED_TIE_SHARE, ties
    y, am = run_stem_forward(backend(who), SATURATED, "saturated", alpha)
    _record(who, "stem forward", judge_stem_forward(who, f"stem forward saturated alpha {alpha}", y, am, r, alpha, True))


def check_stem_rejections(who):
    be = backend(who)
    big = [be.put(np.zeros(1 << 16, np.float32)) for _ in range(5)]                 # (room for the one legal call below)
    p = [q for _, q in big]
    assert be.call("depth_stem_forward", *p, 1, 58, 87, 1.0) == 0
    for n, ih, iw in ((1, 58, 127), (1, 5, 87), (1, 58, 5), (0, 58, 87)):
        assert be.call("depth_stem_forward", *p, n, ih, iw, 1.0) == E_ARG, (who, n, ih, iw)


# ------------------------------------------------------------------------------------------------------------------------ stem backward
STEM_BWD = [(1100, 13, 18), (400, 42, 10), (1024, 6, 6), (1025, 6, 6), (1, 6, 6), (1, 6, 18), (3, 58, 87)]


@functools.lru_cache(None)
def stem_bwd_data(shape, kind):
    n, ih, iw = shape
    ph, pw = ref.pooled_size(ih, iw)
    rng = np.random.default_rng([n, ih, iw, 7, len(kind)])
    am = rng.integers(0, 4, (n, ph, pw, 32)).astype(np.uint8)
    if kind == "real":
        img, g = rng.uniform(-0.5, 1.5, shape), rng.standard_normal((n, ph, pw, 32))
    else:
        img, g = rng.integers(-2, 3, shape), rng.integers(-2, 3, (n, ph, pw, 32))
    return np.ascontiguousarray(img, np.float32), am, np.ascontiguousarray(g, np.float32)


@functools.lru_cache(None)
def stem_bwd_ref(shape, kind):
    return ref.stem_backward(*stem_bwd_data(shape, kind))


def run_stem_backward(be, shape, kind):
    n, ih, iw = shape
    keep = [be.put(a) for a in stem_bwd_data(shape, kind)]
    nb = be.size("depth_stem_backward_scratch_bytes")
    outs = []
    for _ in range(2):
        out, sc = Guarded(be, ref.STEM_WB * 4), Guarded(be, nb)
        assert be.call("depth_stem_backward", *[p for _, p in keep], out.ptr, n, ih, iw, sc.ptr, nb) == 0
        sc.read(np.int32, (-1,), "stem backward scratch")
        outs.append(out.read(np.float32, (ref.STEM_WB,), "stem grad_wb"))
    assert np.array_equal(outs[0].view(np.int32), outs[1].view(np.int32)), f"{be.who}: stem backward {shape}: two calls differ"
    return outs[0]


def check_stem_backward(who, shape):
    be = backend(who)
    tag = f"stem backward {shape}"
    bit_equal(who, tag + " exact", run_stem_backward(be, shape, "exact"), stem_bwd_ref(shape, "exact").val)
    _record(who, "stem backward", within(who, tag + " real", run_stem_backward(be, shape, "real"), stem_bwd_ref(shape, "real")))


# ------------------------------------------------------------------------------------------------------------------------ ELU' + pad
PAD_CHANNELS = (4, 32, 68)


def pad_shapes(pad):
    """(n, oh, ow): one whose padded pixel count is a multiple of 256 (so is the element count, and the kernel's count of 16-byte pieces), one odd"""
    full = (4, 8 - 2 * pad, 8 - 2 * pad) if pad < 4 else (1, 8, 8)
    assert (full[0] * (full[1] + 2 * pad) * (full[2] + 2 * pad)) % 256 == 0
    return full, (3, 5, 7)


def check_pad(who, pad, act):
    be = backend(who)
    for c in PAD_CHANNELS:
        for n, oh, ow in pad_shapes(pad):
            rng = np.random.default_rng([pad, act, c, n])
            y = ref.elu64(2.0 * rng.standard_normal((n, oh, ow, c)), ALPHA).astype(np.float32)
            y[rng.random(y.shape) < 0.1] = 0.0
            g = rng.standard_normal(y.shape).astype(np.float32)
            assert (y > 0).any() and (y < 0).any() and (y == 0).any()
            assert ((n * (oh + 2 * pad) * (ow + 2 * pad) * c) % 256 == 0) == ((n, oh, ow) != (3, 5, 7))
            want, want_p = ref.elu_backward_pad(g, y, pad, act, ALPHA)
            keep = [be.put(g), be.put(y)]
            dy, dyp = Guarded(be, want.size * 4), Guarded(be, want_p.size * 4)
            assert be.call("elu_backward_pad", keep[0][1], keep[1][1], dy.ptr, dyp.ptr, n, oh, ow, c, pad, act, ALPHA) == 0
            tag = f"{who}: pad {pad} act {act} channels {c} {(n, oh, ow)}"
            got, got_p = dy.read(np.int32, want.shape, "grad_pre"), dyp.read(np.int32, want_p.shape, "grad_pre_padded")
            assert np.array_equal(got, want.view(np.int32)), tag
            assert np.array_equal(got_p, want_p.view(np.int32)), tag
            border = np.ones(want_p.shape, bool)
            border[:, pad:pad + oh, pad:pad + ow] = False
            assert (got_p[border] == 0).all(), tag + ": a border element is not +0"
    _record(who, "pad", 0.0)                             # bit for bit: no error to relate to a bound


# ------------------------------------------------------------------------------------------------------------------------ window GEMMs
CONV_SHAPES = [(1, 1, 258, 16, 4, 1, 2), (2, 18, 17, 64, 36, 2, 2), (3, 20, 19, 128, 68, 3, 5), (5, 17, 18, 16, 132, 1, 2), (8, 18, 17, 16, 16, 2, 2),
               (1, 27, 41, 32, 64, 3, 3)]
BWD_INPUT_SHAPES = [s for s in CONV_SHAPES if s[4] >= 16 and not s[4] & (s[4] - 1)]
WGRAD_CAP = (800, 1, 258, 16, 4, 1, 2)
CONFIGS = (2, 3, 4)
_cid = lambda s: "x".join(map(str, s))


@functools.lru_cache(None)
def conv_data(shape, kind):
    """x [n][ih][iw][cin] (real: ELU outputs), weight [cout][kh][kw][cin], bias [cout], gradient at the output [n][oh][ow][cout]"""
    n, ih, iw, cin, cout, kh, kw = shape
    oh, ow = ih - kh + 1, iw - kw + 1
    rng = np.random.default_rng(list(shape) + [len(kind)])
    if kind == "real":
        x, w = ref.elu64(rng.standard_normal((n, ih, iw, cin)), ALPHA), 0.1 * rng.standard_normal((cout, kh, kw, cin))
        b, g = 0.1 * rng.standard_normal(cout), rng.standard_normal((n, oh, ow, cout))
    else:
        x, w, b, g = (rng.integers(-2, 3, s) for s in ((n, ih, iw, cin), (cout, kh, kw, cin), (cout,), (n, oh, ow, cout)))
    return tuple(np.ascontiguousarray(a, np.float32) for a in (x, w, b, g))


@functools.lru_cache(None)
def conv_pre_ref(shape, kind, bias):
    x, w, b, _ = conv_data(shape, kind)
    return ref.conv_pre(x, w, b if bias else None)


def force(be, cfg):
    if be.who == "hip":
        be.lib.qa_gemm_force_config.argtypes = [C.c_int32]
        be.lib.qa_gemm_force_config(cfg)


def check_conv_forward(who, shape, cfg=-1):
    be = backend(who)
    n, ih, iw, cin, cout, kh, kw = shape
    oh, ow = ih - kh + 1, iw - kw + 1
    try:
        force(be, cfg)
        for kind in ("real", "exact"):
            x, w, b, _ = conv_data(shape, kind)
            keep = [be.put(a) for a in (x, w, b)]
            for bias in (True, False):
                pre = conv_pre_ref(shape, kind, bias)
                for act in (0, 1, 2):
                    y = Guarded(be, n * oh * ow * cout * 4)
                    assert be.call("conv_nhwc_forward", keep[0][1], keep[1][1], keep[2][1] if bias else None, y.ptr, n, ih, iw, cin, kh, kw, cout, act, ALPHA) == 0
                    got = y.read(np.float32, (n, oh, ow, cout), "conv y")
                    tag = f"conv forward {shape} cfg {cfg} {kind} act {act}" + ("" if bias else " no bias")
                    if kind == "exact":
                        live = pre.val >= 0 if act == 1 else np.ones(pre.val.shape, bool)
                        bit_equal(who, tag, got, np.where(live, ref.act_forward(act, ALPHA, pre.val, 0.0).val, 0.0), live)
                        ratio = within(who, tag, got, ref.act_forward(act, ALPHA, pre.val, 0.0))
                    else:
                        ratio = within(who, tag, got, ref.act_forward(act, ALPHA, *pre))
                    _record(who, "conv forward", ratio)
    finally:
        force(be, -1)


@functools.lru_cache(None)
def bwd_input_data(shape, kind):
    """the forward convolution's gradient at its output padded with kh - 1 / kw - 1 zeros, and its weights flipped: [cin][kh][kw][cout]"""
    n, ih, iw, cin, cout, kh, kw = shape
    _, w, _, g = conv_data(shape, kind)
    gp = np.zeros((n, ih + kh - 1, iw + kw - 1, cout), np.float32)
    gp[:, kh - 1:kh - 1 + g.shape[1], kw - 1:kw - 1 + g.shape[2]] = g
    return gp, np.ascontiguousarray(w[:, ::-1, ::-1, :].transpose(3, 1, 2, 0))


def x_act_for(shape, kind, act):
    """the activation OUTPUT that was the convolution's input: ELU outputs, ReLU outputs (some exactly zero), or none"""
    n, ih, iw, cin = shape[:4]
    rng = np.random.default_rng(list(shape) + [act, len(kind)])
    if act == 0:
        return None
    if kind == "exact":
        assert act == 2
        return rng.integers(0, 3, (n, ih, iw, cin)).astype(np.float32)
    v = rng.standard_normal((n, ih, iw, cin))
    return (ref.elu64(v, ALPHA) if act == 1 else np.maximum(v, 0.0)).astype(np.float32)


def check_conv_backward_input(who, shape, cfg=-1):
    be = backend(who)
    n, ih, iw, cin, cout, kh, kw = shape
    try:
        force(be, cfg)
        for kind, acts in (("real", (0, 1, 2)), ("exact", (0, 2))):            # (an ELU output is no small integer: depth_stem_ref, "the exact pass")
            gp, wf = bwd_input_data(shape, kind)
            keep = [be.put(gp), be.put(wf)]
            for act in acts:
                xa = x_act_for(shape, kind, act)
                kx = be.put(xa) if xa is not None else (None, None)
                out = Guarded(be, n * ih * iw * cin * 4)
                assert be.call("conv_nhwc_backward_input", keep[0][1], keep[1][1], kx[1], out.ptr, n, gp.shape[1], gp.shape[2], cout, kh, kw, cin, act, ALPHA) == 0
                got = out.read(np.float32, (n, ih, iw, cin), "conv grad_in")
                tag = f"conv backward-input {shape} cfg {cfg} {kind} act {act}"
                r = ref.conv_backward_input(gp, wf, xa, act, ALPHA)
                if kind == "exact":
                    bit_equal(who, tag, got, r.val)
                else:
                    _record(who, "conv backward-input", within(who, tag, got, r))
    finally:
        force(be, -1)


@functools.lru_cache(None)
def wgrad_ref(shape, kind):
    x, _, _, g = conv_data(shape, kind)
    return ref.conv_backward_weight(x, g, shape[5], shape[6])


def run_conv_backward_weight(be, shape, kind):
    n, ih, iw, cin, cout, kh, kw = shape
    x, _, _, g = conv_data(shape, kind)
    keep = [be.put(x), be.put(g)]
    nb = be.size("conv_nhwc_backward_weight_scratch_bytes", n, ih, iw, cin, kh, kw, cout)
    assert nb > 0
    outs = []
    for _ in range(2):
        gw, gb, sc = Guarded(be, cout * kh * kw * cin * 4), Guarded(be, cout * 4), Guarded(be, nb)
        assert be.call("conv_nhwc_backward_weight", keep[0][1], keep[1][1], gw.ptr, gb.ptr, n, ih, iw, cin, kh, kw, cout, sc.ptr, nb) == 0
        sc.read(np.int32, (-1,), "conv backward-weight scratch")
        outs.append((gw.read(np.float32, (cout, kh, kw, cin), "conv grad_weight"), gb.read(np.float32, (cout,), "conv grad_bias")))
    for a, b in zip(*outs):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), f"{be.who}: conv backward-weight {shape}: two calls differ"
    return outs[0]


def check_conv_backward_weight(who, shape, cfg=-1, kinds=("exact", "real")):
    be = backend(who)
    try:
        force(be, cfg)
        for kind in kinds:
            gw, gb = run_conv_backward_weight(be, shape, kind)
            rw, rb = wgrad_ref(shape, kind)
            tag = f"conv backward-weight {shape} cfg {cfg} {kind}"
            if kind == "exact":
                bit_equal(who, tag, gw, rw.val)
                bit_equal(who, tag + " bias", gb, rb.val)
            else:
                _record(who, "conv backward-weight", max(within(who, tag, gw, rw), within(who, tag + " bias", gb, rb)))
    finally:
        force(be, -1)


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_cases_are_what_they_claim():
    """from the kernels' constants as the headers state them: 1,024 workgroups at most, bands of 9 pooled rows, 8 pooled pixels per pass of a workgroup,
    more than 256 output pixels per image, a split of at most 192"""
    items = lambda s: s[0] * -(-ref.pooled_size(s[1], s[2])[0] // ref.STEM_BAND)
    assert [items(s) for s in STEM_BWD[:4]] == [1100, 1200, 1024, 1025]
    assert [ref.pooled_size(*s[1:]) for s in ((1, 6, 6), (1, 6, 18))] == [(1, 1), (1, 7)]
    assert sorted({ref.pooled_size(ih, iw)[0] for _, ih, iw in STEM_SHAPES}) == [1, 9, 10, 18, 19, 27]
    assert {iw for _, _, iw in STEM_SHAPES} >= {6, 126} and any(iw % 2 for _, _, iw in STEM_SHAPES)
    assert set(np.unique(stem_bwd_data((3, 58, 87), "real")[1])) == {0, 1, 2, 3}
    n, ih, iw, cin, cout, kh, kw = CONV_SHAPES[0]
    assert (ih - kh + 1) * (iw - kw + 1) == 257
    n, ih, iw, cin, cout, kh, kw = CONV_SHAPES[4]
    assert n * (ih - kh + 1) * (iw - kw + 1) == 17 * 128
    assert [s[4] for s in BWD_INPUT_SHAPES] == [16, 64]
    # the capped split: 205,600 pixels in 192 slabs of one 32 x 4 product and one bias row each (qa_gemm.hip, conv_wgrad_plan and the scratch layout)
    n, ih, iw, cin, cout, kh, kw = WGRAD_CAP
    assert n * (ih - kh + 1) * (iw - kw + 1) == 205600
    nb = _capi.load_library().qa_conv_nhwc_backward_weight_scratch_bytes(*WGRAD_CAP[:4], kh, kw, cout)
    assert nb == 192 * (kh * kw * cin * cout + cout) * 4, nb


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("shape", STEM_SHAPES, ids=_cid)
def test_reference_leaves_few_argmax_undecided(shape, alpha):
    share = undecided_share(stem_ref(shape, "real", alpha))
    print("MEASURED undecided share", shape, "%.5f %%" % (100 * share))
    assert share <= ref.UNDECIDED_CAP


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("shape", STEM_SHAPES, ids=_cid)
def test_twin_stem_forward(shape, alpha):
    check_stem_forward("twin", shape, alpha)


@pytest.mark.parametrize("alpha", ALPHAS)
def test_twin_stem_forward_on_a_saturated_image(alpha):
    check_stem_saturated("twin", alpha)


def test_twin_stem_rejections():
    check_stem_rejections("twin")


@pytest.mark.parametrize("shape", STEM_BWD, ids=_cid)
def test_twin_stem_backward(shape):
    check_stem_backward("twin", shape)


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("pad", [0, 1, 4])
def test_twin_elu_backward_pad(pad, act):
    check_pad("twin", pad, act)


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=_cid)
def test_twin_conv_forward(shape):
    check_conv_forward("twin", shape)


@pytest.mark.parametrize("shape", BWD_INPUT_SHAPES, ids=_cid)
def test_twin_conv_backward_input(shape):
    check_conv_backward_input("twin", shape)


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=_cid)
def test_twin_conv_backward_weight(shape):
    check_conv_backward_weight("twin", shape)


def test_twin_conv_backward_weight_over_205600_pixels():
    check_conv_backward_weight("twin", WGRAD_CAP, kinds=("exact",))


# ---- teeth: the twin's own output against a reference with one deliberate defect must fail the comparison
TEETH_STEM = (3, 58, 87)
TEETH_CONV = (1, 27, 41, 32, 64, 3, 3)


@pytest.mark.parametrize("kind", ["real", "exact"])
def test_teeth_stem_forward_with_a_tap_zeroed(kind):
    img, w, b = stem_data(TEETH_STEM, kind)
    y, am = run_stem_forward(backend("twin"), TEETH_STEM, kind, ALPHA)
    judge_stem_forward("twin", "intact", y, am, stem_ref(TEETH_STEM, kind, ALPHA), ALPHA, kind == "exact")
    w2 = w.copy()
    w2[:, 13] = 0.0
    with pytest.raises(AssertionError):
        judge_stem_forward("twin", "a tap zeroed", y, am, ref.stem_forward(img, w2, b, ALPHA), ALPHA, kind == "exact")


def test_teeth_stem_forward_with_the_last_maximum_rule():
    y, am = run_stem_forward(backend("twin"), SATURATED, "saturated", ALPHA)
    judge_stem_forward("twin", "intact", y, am, stem_ref(SATURATED, "saturated", ALPHA), ALPHA, True)
    with pytest.raises(AssertionError, match="first-maximum"):
        judge_stem_forward("twin", "last maximum", y, am, ref.stem_forward(*stem_data(SATURATED, "saturated"), ALPHA, defect="last"), ALPHA, True)


@pytest.mark.parametrize("kind", ["real", "exact"])
def test_teeth_stem_backward_with_a_band_skipped(kind):
    """one image's last band: three of its 27 pooled rows.  On the real pass the defect is judged where the bound has teeth, on this small case"""
    got = run_stem_backward(backend("twin"), TEETH_STEM, kind)
    broken = ref.stem_backward(*stem_bwd_data(TEETH_STEM, kind), skip_band=(1, 2))
    if kind == "exact":
        bit_equal("twin", "intact", got, stem_bwd_ref(TEETH_STEM, kind).val)
        with pytest.raises(AssertionError):
            bit_equal("twin", "a band skipped", got, broken.val)
    else:
        within("twin", "intact", got, stem_bwd_ref(TEETH_STEM, kind))
        with pytest.raises(AssertionError):
            within("twin", "a band skipped", got, broken)


@pytest.mark.parametrize("kind", ["real", "exact"])
def test_teeth_conv_forward_with_a_tap_zeroed(kind):
    n, ih, iw, cin, cout, kh, kw = TEETH_CONV
    be = backend("twin")
    x, w, b, _ = conv_data(TEETH_CONV, kind)
    out = np.zeros((n, ih - kh + 1, iw - kw + 1, cout), np.float32)
    assert be.call("conv_nhwc_forward", be.put(x)[1], be.put(w)[1], be.put(b)[1], C.c_void_p(out.ctypes.data), n, ih, iw, cin, kh, kw, cout, 0, ALPHA) == 0
    within("twin", "intact", out, ref.conv_forward(x, w, b, 0, ALPHA))
    w2 = w.copy()
    w2[:, 1, 2, :] = 0.0
    with pytest.raises(AssertionError):
        within("twin", "a tap zeroed", out, ref.conv_forward(x, w2, b, 0, ALPHA))
    if kind == "exact":
        with pytest.raises(AssertionError):
            bit_equal("twin", "a tap zeroed", out, ref.conv_forward(x, w2, b, 0, ALPHA).val)


def test_teeth_conv_backward_weight_with_a_row_skipped():
    x, _, _, g = conv_data(TEETH_CONV, "exact")
    gw, gb = run_conv_backward_weight(backend("twin"), TEETH_CONV, "exact")
    bit_equal("twin", "intact", gw, wgrad_ref(TEETH_CONV, "exact")[0].val)
    bw, bb = ref.conv_backward_weight(x, g, 3, 3, skip_row=(0, g.shape[1] - 1))
    with pytest.raises(AssertionError):
        bit_equal("twin", "a row skipped", gw, bw.val)
    with pytest.raises(AssertionError):
        bit_equal("twin", "a row skipped, bias", gb, bb.val)


# ------------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("shape", STEM_SHAPES, ids=_cid)
def test_hip_stem_forward(shape, alpha):
    check_stem_forward("hip", shape, alpha)


@pytest.mark.gpu
@pytest.mark.parametrize("alpha", ALPHAS)
def test_hip_stem_forward_on_a_saturated_image(alpha):
    check_stem_saturated("hip", alpha)


@pytest.mark.gpu
def test_hip_stem_rejections():
    check_stem_rejections("hip")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", STEM_BWD, ids=_cid)
def test_hip_stem_backward(shape):
    check_stem_backward("hip", shape)


@pytest.mark.gpu
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("pad", [0, 1, 4])
def test_hip_elu_backward_pad(pad, act):
    check_pad("hip", pad, act)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=_cid)
def test_hip_conv_forward(shape, cfg):
    check_conv_forward("hip", shape, cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("shape", BWD_INPUT_SHAPES, ids=_cid)
def test_hip_conv_backward_input(shape, cfg):
    check_conv_backward_input("hip", shape, cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=_cid)
def test_hip_conv_backward_weight(shape, cfg):
    check_conv_backward_weight("hip", shape, cfg)


@pytest.mark.gpu
def test_hip_conv_backward_weight_at_the_split_cap():
    check_conv_backward_weight("hip", WGRAD_CAP, kinds=("exact",))
