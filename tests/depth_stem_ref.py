"""A float64 statement of the depth encoder's image stem, written from the contract of include/qa_sim.h ("Image stem of the vision student's depth
encoder") and the header of csrc/qa_conv.hip, and from nothing else: plain numpy over channels-last tensors, no tiles, no bands, no slabs, no GPU.

    stem_forward            Conv 5x5 (1 -> 32) + bias, max-pool 2x2 (floor mode, FIRST maximum in row-major window order), ELU(alpha)
    stem_backward           the 800 weight + 32 bias sums of that convolution through a GIVEN argmax
    elu_backward_pad        grad_out * act'(y), plain and with a zero border -- in fp32, operation by operation (the entry is elementwise: it is
                            compared bit for bit, it needs no bound)
    conv_forward / conv_backward_input / conv_backward_weight      the "valid", stride 1 window GEMMs; act 0 none, 1 ELU(alpha), 2 ReLU

Every result is a `Res(val, err)`: the float64 value and, elementwise, an ABSOLUTE worst-case bound on |what an fp32 evaluation may give - val|,
computed in float64 with u = U = 2^-23 (ONE ulp, not half: an accumulator that truncates instead of rounding is covered).  The rules:

  sum of K products plus a bias     err = (K + 2) u (sum |a| |b| + |bias|): K roundings of the running sum, one of the bias addition and one to
                                    spare, each at most u times the sum of magnitudes -- in ANY summation order, with or without fused multiply-adds
                                    or a wider accumulator.  K is 25 for the stem, kh kw cin for the window GEMMs forward and backward-input, the
                                    number of pooled / output pixels summed over for the weight and bias gradients.
  max over the pool's four cells    |max_i a_i - max_i b_i| <= max_i |a_i - b_i|: the pooled value carries the LARGEST of its four cells' bounds.
  ReLU                              Lipschitz 1: the bound passes through.
  ELU(alpha)                        err = max(1, alpha) err_pre + 4 u |y|, plus an absolute 4 u alpha where the pre-activation is negative
                                    (expf(x) - 1 cancels near 0: its error is relative to e^x <= 1, not to the difference).
  times act'(x_act)                 (backward-input) x_act is an exact fp32 tensor; d = 1 | x + alpha | 0 with e_d = u (|x| + alpha) where the sum is
                                    formed, else 0; err' = |d| err_p + (|p| + err_p) e_d, err = err' + u (|p d| + err'): the product rule, then the
                                    rounding of the product.

The pool's argmax is judged with the same bounds (`StemFwd.candidates`): a cell is a candidate for the maximum unless the float64 best cell beats it by
more than the sum of their two bounds.  One candidate: the argmax is DECIDED and must be that cell.  Several ("undecided"): fp32 may pick any of them;
their share is capped at UNDECIDED_CAP per case, and the cap is asserted on the reference before a kernel is judged.

THE EXACT PASS.  The worst-case bound has no teeth on long reductions (over 205,600 pixels it exceeds the result).  So every reduction is also run on
small-integer operands: images, activations, weights and gradients from {-2..2} (multiples of 1/8 and 1/16 for the stem forward).  Every product and
every partial sum is then exactly representable in fp32, in any summation order, so the kernel's result must be BIT-EQUAL to the float64 value cast to
fp32 -- a dropped, doubled or misplaced term cannot hide.  Where the problem ends in an ELU this holds where its pre-activation is >= 0; the negative
entries are compared with the ELU rule above on an exact pre-activation.  Input gradients taken against ELU outputs run the exact pass with act 0
(ReLU where the case calls for act 2): an ELU output is no small integer.  On the exact pass the argmax has no undecided cells: it must equal the
first-maximum rule everywhere, ties included.  `exact_bits` gives the fp32 bit patterns to compare with.

The `defect` arguments exist for the tests that show the comparisons have teeth (a tap zeroed is done by the caller on the weights): "last" applies
the LAST-maximum rule, `skip_band=(image, band)` leaves one 9-row band of one image out of the backward sums.  Test infrastructure only."""
from collections import namedtuple

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

U = 2.0 ** -23
UNDECIDED_CAP = 1.0e-3                  # share of pooled outputs whose argmax fp32 cannot decide, per case (uniform images: the reference's own is <= 0.026 %)
SATURATED_TIE_SHARE = 0.3               # a clipped image's share of pooled outputs whose maximum is attained by more than one cell
STEM_C, STEM_K, STEM_BAND = 32, 5, 9
STEM_TAPS = STEM_K * STEM_K
STEM_WB = STEM_C * STEM_TAPS + STEM_C

Res = namedtuple("Res", "val err")
StemFwd = namedtuple("StemFwd", "y arg cells cells_err pre candidates")          # y: Res; pre: Res of the pooled pre-activation; cells [n][ph][pw][4][32]


def f64(a):
    return np.asarray(a, np.float64)


def exact_bits(val):
    """the fp32 bit patterns of a float64 array whose every element is exactly representable in fp32"""
    v32 = f64(val).astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), val), "the exact pass left the fp32 grid"
    return v32.view(np.int32)


def pooled_size(ih, iw):
    return (ih - STEM_K + 1) // 2, (iw - STEM_K + 1) // 2


def elu64(v, alpha):
    return np.where(v > 0, v, alpha * np.expm1(np.minimum(v, 0.0)))


def act_forward(act, alpha, pre, err):
    """-> Res of act(pre) from the pre-activation and its bound"""
    if act == 0:
        return Res(pre, err)
    if act == 2:
        return Res(np.maximum(pre, 0.0), err)
    assert act == 1
    y = elu64(pre, alpha)
    return Res(y, max(1.0, alpha) * err + 4 * U * np.abs(y) + np.where(pre < 0, 4 * U * alpha, 0.0))


def act_derivative(act, alpha, y):
    """-> (d, e_d) of the derivative from the activation's fp32 OUTPUT y"""
    y = f64(y)
    if act == 1:
        return np.where(y > 0, 1.0, y + alpha), np.where(y > 0, 0.0, U * (np.abs(y) + abs(alpha)))
    if act == 2:
        return np.where(y > 0, 1.0, 0.0), np.zeros_like(y)
    assert act == 0
    return np.ones_like(y), np.zeros_like(y)


# --------------------------------------------------------------------------------------------------------------------------- the stem
def _stem_windows(images):
    """[n][ih][iw] -> [n][2 ph][2 pw][25]: the 5x5 window at every convolution output the pool reads"""
    img = f64(images)
    n, ih, iw = img.shape
    ph, pw = pooled_size(ih, iw)
    win = sliding_window_view(img, (STEM_K, STEM_K), axis=(1, 2))[:, :2 * ph, :2 * pw]
    return win.reshape(n, 2 * ph, 2 * pw, STEM_TAPS), ph, pw


def _cells(a, ph, pw):
    """[n][2 ph][2 pw][c] -> [n][ph][pw][4][c], cell d = 2 dy + dx"""
    n, c = a.shape[0], a.shape[-1]
    return a.reshape(n, ph, 2, pw, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, ph, pw, 4, c)


def stem_forward(images, weight, bias, alpha, defect=None):
    win, ph, pw = _stem_windows(images)
    w, b = f64(weight).reshape(STEM_C, STEM_TAPS), f64(bias)
    cells = _cells(win @ w.T + b, ph, pw)
    cells_err = _cells((STEM_TAPS + 2) * U * (np.abs(win) @ np.abs(w).T + np.abs(b)), ph, pw)
    if defect == "last":
        arg = 3 - cells[:, :, :, ::-1].argmax(3)
    else:
        assert defect is None
        arg = cells.argmax(3)                                                   # numpy: the first of equal maxima
    best = np.take_along_axis(cells, arg[:, :, :, None], 3)
    best_err = np.take_along_axis(cells_err, arg[:, :, :, None], 3)
    candidates = best - cells <= best_err + cells_err                           # (the best cell itself: 0 <= 2 e)
    pre = Res(best[:, :, :, 0], cells_err.max(3))
    return StemFwd(act_forward(1, alpha, *pre), arg.astype(np.uint8), cells, cells_err, pre, candidates)


def stem_backward(images, argmax, grad_pre, skip_band=None):
    """-> Res over the 832 sums: [c][ky][kx] then the 32 bias sums"""
    win, ph, pw = _stem_windows(images)
    n = win.shape[0]
    g = f64(grad_pre).copy()
    if skip_band is not None:
        im, band = skip_band
        g[im, band * STEM_BAND:(band + 1) * STEM_BAND] = 0.0
    wc = _cells(win, ph, pw)                                                    # [n][ph][pw][4][25]
    val, mag = np.zeros((STEM_C, STEM_TAPS)), np.zeros((STEM_C, STEM_TAPS))
    for d in range(4):
        gd = np.where(argmax == d, g, 0.0).reshape(-1, STEM_C)
        wd = wc[:, :, :, d].reshape(-1, STEM_TAPS)
        val += gd.T @ wd
        mag += np.abs(gd).T @ np.abs(wd)
    k = n * ph * pw
    g2 = g.reshape(-1, STEM_C)
    return Res(np.concatenate([val.reshape(-1), g2.sum(0)]), (k + 2) * U * np.concatenate([mag.reshape(-1), np.abs(g2).sum(0)]))


# --------------------------------------------------------------------------------------------------------------------------- ELU' + pad
def elu_backward_pad(grad_out, y, pad, act, alpha):
    """-> (grad_pre, grad_pre_padded) as fp32 arrays, every operation rounded to fp32 as the header writes it"""
    g, y = np.asarray(grad_out, np.float32), np.asarray(y, np.float32)
    one, zero = np.float32(1.0), np.float32(0.0)
    if act == 1:
        d = np.where(y > 0, one, y + np.float32(alpha))
    elif act == 2:
        d = np.where(y > 0, one, zero)
    else:
        assert act == 0
        d = np.ones_like(y)
    dy = (g * d).astype(np.float32)
    n, oh, ow, c = dy.shape
    dyp = np.zeros((n, oh + 2 * pad, ow + 2 * pad, c), np.float32)
    dyp[:, pad:pad + oh, pad:pad + ow] = dy
    return dy, dyp


# --------------------------------------------------------------------------------------------------------------------------- window GEMMs
def _windows(x, kh, kw):
    """[n][ih][iw][c] -> ([pixels][kh kw c] (tap-major, channel fastest), (n, oh, ow))"""
    x = f64(x)
    n, ih, iw, c = x.shape
    win = sliding_window_view(x, (kh, kw), axis=(1, 2)).transpose(0, 1, 2, 4, 5, 3)          # [n][oh][ow][kh][kw][c]
    oh, ow = ih - kh + 1, iw - kw + 1
    return win.reshape(n * oh * ow, kh * kw * c), (n, oh, ow)


def conv_pre(x, weight, bias):
    """-> Res of the pre-activation [n][oh][ow][cout]; weight [cout][kh][kw][cin]"""
    cout, kh, kw, cin = weight.shape
    win, (n, oh, ow) = _windows(x, kh, kw)
    w = f64(weight).reshape(cout, -1)
    b = np.zeros(cout) if bias is None else f64(bias)
    val = win @ w.T + b
    err = (kh * kw * cin + 2) * U * (np.abs(win) @ np.abs(w).T + np.abs(b))
    return Res(val.reshape(n, oh, ow, cout), err.reshape(n, oh, ow, cout))


def conv_forward(x, weight, bias, act, alpha):
    return act_forward(act, alpha, *conv_pre(x, weight, bias))


def conv_backward_input(grad_padded, weight_flipped, x_act, act_prev, alpha):
    """weight_flipped [cin][kh][kw][cout]; x_act [n][ihp - kh + 1][iwp - kw + 1][cin] (ignored for act_prev 0)"""
    p, e_p = conv_pre(grad_padded, weight_flipped, None)
    if act_prev == 0:
        return Res(p, e_p)
    d, e_d = act_derivative(act_prev, alpha, x_act)
    e = np.abs(d) * e_p + (np.abs(p) + e_p) * e_d
    return Res(p * d, e + U * (np.abs(p * d) + e))


def conv_backward_weight(x, grad_out, kh, kw, skip_row=None):
    """-> (Res grad_weight [cout][kh][kw][cin], Res grad_bias [cout]); `skip_row=(image, oy)` leaves one output row out (a defect for the teeth tests)"""
    win, (n, oh, ow) = _windows(x, kh, kw)
    g = f64(grad_out).copy()
    if skip_row is not None:
        g[skip_row[0], skip_row[1]] = 0.0
    cout, cin = g.shape[-1], np.shape(x)[-1]
    g = g.reshape(-1, cout)
    k = g.shape[0]
    gw = Res((g.T @ win).reshape(cout, kh, kw, cin), ((k + 2) * U * (np.abs(g).T @ np.abs(win))).reshape(cout, kh, kw, cin))
    return gw, Res(g.sum(0), (k + 2) * U * np.abs(g).sum(0))
