"""qa_mlp_pack + qa_mlp_forward (csrc/qa_policy.hip) op by op against tests/mlp_program_ref.py, a float64 interpreter of qa_mlp_op programs written from
the contract of include/qa_sim.h, at the shapes the project's own describers never emit: partly filled wavefronts, odd column offsets, padded
k-blocks over poisoned neighbours, every act code, ragged row counts, split and unsplit launches, the two-group launch.

CPU: the oracle's plain-C twin (qo_mlp_*) against the interpreter on every program; that the bounds have teeth; what the library refuses.
-m gpu: the kernels against the interpreter.  Every comparison uses the bound the interpreter carries through the program (mlp_program_ref's
docstring); there is no tolerance literal in this file.  Outputs are allocated with 16 extra rows and a row stride wider than the op writes, filled
with a sentinel bit pattern: every element the program does not write must come back bit-identical.

Largest err / bound per group on an MI355X (bound = the carried worst-case bound, so ratios far below 1 are expected): NOT MEASURED YET -- the GPU
part of this file has not run on an MI355X; `pytest -m gpu -s tests/test_mlp_ops.py` prints them ("MEASURED worst err/bound so far, <group>").
The twin against the same bounds, on the CPU (same programs): every group's largest ratio is below 0.1.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from quadrupedal_agility_amd import _capi
from tests import mlp_program_ref as ref
from tests.oracle_lib import load_oracle

COLS = _capi.MLP_BUF_COLS
SENTINEL = 0x7FC5A5A5                       # a quiet NaN's bits: no arithmetic produces it, any store over it shows
POISON = 1e30                               # finite: times a zero weight it is zero
E_ARG = -1                                  # QA_E_ARG
ROWS = (1, 15, 16, 17, 33, 2049)           # <= 33: split over strands; 2049: 129 tiles, unsplit, one live row in the last tile


def qa():
    return _capi.load_library()


# ------------------------------------------------------------------------------------------------------------------------ programs
class Prog:
    """an op list with its unpacked weights; packed offsets are laid out with the library's own size function"""

    def __init__(self):
        self.ops, self.w, self.b, self.end = [], [], [], 0

    def _add(self, w=None, b=None, **kw):
        self.ops.append(_capi.QaMlpOp(**kw)); self.w.append(w); self.b.append(b)
        return self

    def copy(self, src, scol, dst, dcol, n, save=None):
        kw = dict(flags=ref.F_SAVE, out_index=save[0], out_col=save[1]) if save else {}
        return self._add(kind=ref.COPY, src_buf=src, src_col=scol, dst_buf=dst, dst_col=dcol, n=n, **kw)

    def load(self, aux, dst, dcol, n, save=None):
        kw = dict(flags=ref.F_SAVE, out_index=save[0], out_col=save[1]) if save else {}
        return self._add(kind=ref.LOAD, dst_buf=dst, dst_col=dcol, n=n, aux_index=aux[0], aux_col=aux[1], **kw)

    def grad(self, src, scol, dst, dcol, n, act=0, aux=(0, 0), add=False, save=None):
        kw = dict(out_index=save[0], out_col=save[1]) if save else {}
        return self._add(kind=ref.GRAD, src_buf=src, src_col=scol, dst_buf=dst, dst_col=dcol, n=n, act=act, aux_index=aux[0], aux_col=aux[1],
                         flags=(ref.F_ADD if add else 0) | (ref.F_SAVE if save else 0), **kw)

    def layer(self, src, scol, k, dst, dcol, n, act, w, b, out=None, save=None, aux=(0, 0), transposed=False, w_off=None):
        op = _capi.QaMlpOp(kind=ref.LAYER, src_buf=src, src_col=scol, dst_buf=dst, dst_col=dcol, k=k, n=n, act=act, aux_index=aux[0], aux_col=aux[1],
                           flags=(ref.F_SAVE if save else 0) | (ref.F_TRANSPOSED if transposed else 0))
        op.out_index, op.out_col = (out if dst < 0 else save) or (0, 0)
        one = (_capi.QaMlpOp * 1)(op)
        one[0].w_off = self.end if w_off is None else w_off
        one[0].b_off = 0
        one[0].b_off = qa().qa_mlp_packed_floats(one, 1)               # the bias goes behind the (padded) weights ...
        self.end = qa().qa_mlp_packed_floats(one, 1)                   # ... and the next layer behind the (padded) bias
        self.ops.append(_capi.QaMlpOp.from_buffer_copy(one[0]))
        self.w.append(None if w is None else np.ascontiguousarray(w, np.float32))
        self.b.append(None if b is None else np.ascontiguousarray(b, np.float32))
        return self

    @property
    def n(self):
        return len(self.ops)

    def c_ops(self):
        return (_capi.QaMlpOp * self.n)(*self.ops)


class Case:
    """a program with its inputs: x (rows, x_cols) fp32, `supplied` {slot: fp32 array} read by the program, `widths` {slot: columns} it writes;
    `layout` of the input rows: plain | strided (x_stride > x_cols) | misaligned (base pointer one float into an allocation)"""

    def __init__(self, tag, group, prog, x, supplied=None, widths=None, layout="plain", meta=None):
        self.tag, self.group, self.prog, self.x, self.layout = tag, group, prog, np.ascontiguousarray(x, np.float32), layout
        self.supplied, self.widths, self.meta = supplied or {}, widths or {}, meta or {}
        self.rows, self.x_cols = self.x.shape

    @functools.cached_property
    def reference(self):
        return ref.run(self.prog.ops, self.prog.w, self.prog.b, self.x, self.x_cols, self.supplied, self.widths)

    def with_rows(self, rows):
        return Case(self.tag, self.group, self.prog, self.x[:rows], {s: t[:rows] for s, t in self.supplied.items()}, self.widths, self.layout, self.meta)


def _signs(rng, shape):
    return rng.choice([-1.0, 1.0], size=shape)


def _teeth_data(rng, rows, k, n):
    """|x|, |w|, |b| in [0.5, 1] with random signs: every product term is at least 0.25"""
    return [(rng.uniform(0.5, 1.0, s) * _signs(rng, s)).astype(np.float32) for s in ((rows, k), (n, k), (n,))]


def _smooth_data(rng, rows, k, n):
    """pre-activations in about [-4, 4]: nothing saturates a difference away"""
    return (rng.standard_normal((rows, k)).astype(np.float32), (rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32),
            (0.1 * rng.standard_normal(n)).astype(np.float32))


def _saved_output(rng, code, rows, n):
    """a saved activation for the derivative code: the forward activation's outputs, some exactly zero, some negated (both signs for every code)"""
    y = ref.forward64(code - 3, 2.0 * rng.standard_normal((rows, n)))
    pick = rng.random((rows, n))
    y = np.where(pick < 0.1, 0.0, np.where(pick < 0.2, -np.abs(y), y)).astype(np.float32)
    y[0, 0] = 0.0
    return y


def layer_case(idx, mode, n, k, scol, dcol, ocol, rows, act=0, bias=True, bufs=(1, 2), layout="plain", group="layer act 0"):
    """mode A: LAYER from buffer 0 to a global output.  mode B: COPY into scratch buffer S, LAYER S -> scratch D + SAVE, COPY D -> a third buffer +
    SAVE (what the layer left in LDS).  Every source column outside [scol, scol + k) that a padded k-block can touch (up to 127 columns beyond k,
    and everything before scol) holds +-1e30.  A derivative `act` makes it a TRANSPOSED layer with a saved activation in slot 2 at column 3."""
    rng = np.random.default_rng(1000 + idx)
    deriv = act in ref.GRAD_CODES
    x_live, w, b = (_teeth_data if act == 0 else _smooth_data)(rng, rows, k, n)
    if not bias or deriv:
        b = None
    if deriv:
        w = np.ascontiguousarray(w.T)                    # the forward layer's (k, n) matrix
    supplied = {2: np.concatenate([np.full((rows, 3), 7.0, np.float32), _saved_output(rng, act, rows, n)], axis=1)} if deriv else {}
    kw = dict(aux=(2, 3), transposed=True) if deriv else {}
    p = Prog()
    if mode == "A":
        x_cols = 671 if (k == 671 and scol == 0) else min(COLS[0], scol + k + 128)
        x = (POISON * _signs(rng, (rows, x_cols))).astype(np.float32)
        live = min(k, x_cols - scol)                     # scol + k may reach into the four padding columns, which read as zero
        x[:, scol:scol + live] = x_live[:, :live]
        p.layer(0, scol, k, -1, 0, n, act, w, b, out=(0, ocol), **kw)
        widths = {0: ocol + n}
    else:
        S, D = bufs
        T = 6 - S - D
        x_cols = min(COLS[0], k + 128)
        x = (POISON * _signs(rng, (rows, x_cols))).astype(np.float32)
        x[:, :k] = x_live
        p.copy(0, 0, S, scol, k)
        if scol:
            p.copy(0, k, S, 0, scol)
        tail = min(x_cols - k, COLS[S] - scol - k)
        if tail > 0:
            p.copy(0, k, S, scol + k, tail)
        p.layer(S, scol, k, D, dcol, n, act, w, b, save=(0, ocol), **kw)
        m = min(n, COLS[T])
        p.copy(D, dcol, T, 0, m, save=(1, 1))
        widths = {0: ocol + n, 1: 1 + m}
    tag = f"{mode} {k}->{n} act {act} src@{scol} dst@{dcol} out@{ocol} {rows} rows {layout}" + ("" if bias else " no bias") + (f" bufs {bufs}" if mode == "B" else "")
    return Case(tag, group, p, x, supplied, widths, layout, dict(mode=mode, n=n, k=k, scol=scol, dcol=dcol, ocol=ocol, act=act, bias=b is not None, x_live_col=scol if mode == "A" else 0))


N_SET = (1, 15, 16, 17, 100, 136, 200, 264, 500, 512)              # nt = 1, 1, 1, 2, 7, 9, 13, 17, 32 (partial last tile), 32
K_SET = (1, 3, 4, 5, 15, 16, 17, 57, 127, 128, 129, 671, 800)      # across both roundings of the k-block count (prefetch depth 8 and 4)
LAYOUTS = ("plain", "strided", "misaligned")


def _act0_table():
    """26 cases: every k twice, every n at least twice; the mode, offsets, row count, bias and input layout rotate"""
    out = []
    for i in range(2 * len(K_SET)):
        k = K_SET[i // 2]
        n = N_SET[(i * 3 + i // 2) % len(N_SET)]
        rows = ROWS[i % len(ROWS)]
        mode = "A" if (k > 128 or i % 2 == 0) else "B"
        scol = (0, 4, 36)[i % 3]
        dcol, ocol = (0, 1, 3, 13)[i % 4], (13, 0, 1, 3)[(i // 2) % 4]
        bufs = (2, 1) if n + dcol > COLS[2] else (1, 2)
        if k == 800 and i % 2 == 1:
            scol = 4                                     # src_col + k = QA_MLP_BUF0_COLS + 4: the last k-block ends in the padding columns
        elif k == 671 and i % 2 == 0:
            scol = 0                                     # x_cols = 671: the rollout's observation row, read to its last column
        elif mode == "A":
            scol = min(scol, (COLS[0] - k) // 4 * 4)
        if mode == "B" and k == 57:
            bufs, scol = (3, 1), 4                       # the last buffer: its padded k-blocks end exactly at the end of LDS
        if mode == "B" and k == 16:
            n, bufs, scol = 512, (3, 1), 36              # ... with a prefetch depth of 4
        out.append(layer_case(i, mode, n, k, scol, dcol, ocol, rows, 0, bias=i % 5 != 0, bufs=bufs, layout=LAYOUTS[i % 3]))
    # the n values the rotation reached once only: a second k each
    seen = {}
    for c in out:
        seen.setdefault(c.meta["n"], set()).add(c.meta["k"])
    extra = [(n, k) for n in N_SET for k in (17, 129) if len(seen.get(n, ())) < 2 and k not in seen.get(n, ())]
    for j, (n, k) in enumerate(extra):
        if len(seen.setdefault(n, set())) >= 2:
            continue
        seen[n].add(k)
        i = len(out)
        out.append(layer_case(i, "AB"[j % 2] if k <= 128 else "A", n, k, (0, 4, 36)[j % 3], (3, 13)[j % 2], (1, 3)[j % 2], ROWS[(j + 2) % len(ROWS)], 0,
                              bufs=(2, 1) if n + 13 > COLS[2] else (1, 2), layout=LAYOUTS[j % 3]))
    return out


def _act_table():
    out = []
    for j, act in enumerate((1, 2, 3, 7, 8, 9)):                    # (code 0: the table above)
        n, k = (100, 136, 17, 264, 200, 15)[j], (127, 57, 128, 16, 5, 129 - 1)[j]
        out.append(layer_case(100 + j, "AB"[j % 2], n, k, (0, 4, 36)[j % 3], (1, 13, 0, 3)[j % 4], (3, 0, 13, 1)[j % 4], ROWS[(j + 1) % len(ROWS)], act,
                              layout=LAYOUTS[(j + 1) % 3], group="layer forward codes"))
    for j, act in enumerate(ref.GRAD_CODES):
        n, k = (200, 100, 264, 17, 136, 500)[j], (12, 57, 100, 128, 5, 64)[j]
        out.append(layer_case(200 + j, "AB"[j % 2], n, k, (4, 0, 36)[j % 3], (0, 3, 13, 1)[j % 4], (1, 13, 3, 0)[j % 4], ROWS[(j + 3) % len(ROWS)], act,
                              bufs=(2, 1) if n > 300 else (1, 2), layout=LAYOUTS[j % 3], group="layer derivative codes"))
    return out


def _elementwise_table():
    """COPY, GRAD (act 0; ADD; every derivative code), LOAD, LOAD + SAVE; slot 0 is written, slot 1 supplies the LOADs, slot 2 the saved activation"""
    out, idx = [], 0
    kinds = ["copy", "grad", "add", "load", "load+save"] + [f"d{c}" for c in ref.GRAD_CODES]
    for n in (1, 29, 127):
        for kind in kinds:
            rng = np.random.default_rng(3000 + idx)
            rows = ROWS[idx % len(ROWS)]
            scol, dcol, ocol, acol = (0, 4, 36)[idx % 3], (0, 1, 3, 13)[idx % 4], (13, 3, 1, 0)[(idx // 2) % 4], (1, 13, 0, 3)[idx % 4]
            dst = 1 + idx % 3
            if dcol + n > COLS[dst]:
                dst = 2
            x = rng.standard_normal((rows, scol + n + 40)).astype(np.float32)
            supplied = {1: rng.standard_normal((rows, acol + n)).astype(np.float32)}
            p = Prog()
            if kind == "copy":
                p.copy(0, scol, dst, dcol, n, save=(0, ocol))
            elif kind == "grad":
                p.grad(0, scol, dst, dcol, n, save=(0, ocol))
            elif kind == "add":
                p.copy(0, scol + 40, dst, dcol, n).grad(0, scol, dst, dcol, n, add=True, save=(0, ocol))
            elif kind == "load":
                p.load((1, acol), dst, dcol, n).copy(dst, dcol, 1 + dst % 3, 0, n, save=(0, ocol))
            elif kind == "load+save":
                p.load((1, acol), dst, dcol, n, save=(0, ocol))
            else:
                code = int(kind[1:])
                supplied[2] = np.concatenate([np.zeros((rows, acol), np.float32), _saved_output(rng, code, rows, n)], axis=1)
                p.copy(0, scol + 40, dst, dcol, n).grad(0, scol, dst, dcol, n, act=code, aux=(2, acol), add=idx % 2 == 0, save=(0, ocol))
            out.append(Case(f"{kind} n {n} src@{scol} dst {dst}@{dcol} out@{ocol} aux@{acol} {rows} rows", "elementwise", p, x, supplied, {0: ocol + n},
                            LAYOUTS[idx % 3]))
            idx += 1
    return out


COMPOSITE_ROWS = 2049
WA, WB = (450, 200, 12), (100, 40, 5)      # column tiles per layer 29, 13, 1 | 7, 3, 1: the two-group launch's four tiles-per-wave branches (8, 4 | 2, 1)
ACT_A, ACT_B = (1, 3), (2, 1)              # ELU, tanh | ReLU, ELU -- codes of the launches without the ABI 17 features


@functools.lru_cache(None)
def _composite_weights():
    rng = np.random.default_rng(77)
    mk = lambda n, k: ((rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32), (0.2 * rng.standard_normal(n)).astype(np.float32))
    return [mk(WA[0], 57), mk(WA[1], WA[0]), mk(WA[2], WA[1])], [mk(WB[0], 61), mk(WB[1], WB[0]), mk(WB[2], WB[1])]


@functools.lru_cache(None)
def composite_forward(saving=False):
    """two independent three-layer stacks sharing the input tile: A reads x[:, 0:57], B reads x[:, 60:121]; outputs 0 and 1.  `saving`: the hidden
    activations also go to the tape (slot 2) at multiples of 4 -- the forward half of a training step (and the saved outputs of the gradient chain)."""
    A, B = _composite_weights()
    x = np.random.default_rng(78).standard_normal((COMPOSITE_ROWS, 125)).astype(np.float32)
    p = Prog()
    sv = (lambda col: dict(save=(2, col))) if saving else (lambda col: {})
    p.layer(0, 0, 57, 1, 0, WA[0], ACT_A[0], *A[0], **sv(0))
    p.layer(1, 0, WA[0], 2, 0, WA[1], ACT_A[1], *A[1], **sv(452))
    p.layer(2, 0, WA[1], -1, 0, WA[2], 0, *A[2], out=(0, 0))
    p.layer(0, 60, 61, 1, 0, WB[0], ACT_B[0], *B[0], **sv(652))
    p.layer(1, 0, WB[0], 3, 0, WB[1], ACT_B[1], *B[1], **sv(752))
    p.layer(3, 0, WB[1], -1, 0, WB[2], 0, *B[2], out=(1, 0))
    widths = {0: WA[2], 1: WB[2]}
    if saving:
        widths[2] = 792
    return Case("two-strand forward chain" + (" with saves" if saving else ""), "composite", p, x, {}, widths, "strided")


TAPE = dict(a1=(0, WA[0]), a2=(452, WA[1]), b1=(652, WB[0]), b2=(752, WB[1]))
GTAPE = dict(a2=(0, WA[1]), a1=(200, WA[0]), ain=(652, 57), gb=(712, WB[2]), b2=(720, WB[1]), b1=(760, WB[0]), bin=(860, 61))


@functools.lru_cache(None)
def composite_backward():
    """the input-gradient chain of composite_forward as train_chain lays such chains out: the input tile is d loss / d output 0, the gradient at
    output 1 arrives in two tensors that are LOADED and added, transposed layers with the derivative of the layer below in their epilogues, every
    pre-activation gradient SAVED to a gradient tape (slot 0) at multiples of 4.  Slot 1: the activation tape, 2 / 3: the two gradients at output 1."""
    A, B = _composite_weights()
    fwd = composite_forward(True).reference[2]
    tape = fwd.val.astype(np.float32)
    rng = np.random.default_rng(79)
    x = (rng.standard_normal((COMPOSITE_ROWS, WA[2])) / 8).astype(np.float32)
    g1, g2 = ((rng.standard_normal((COMPOSITE_ROWS, 1 + WB[2])) / 8).astype(np.float32) for _ in range(2))
    da, db = [c + 3 for c in ACT_A], [c + 3 for c in ACT_B]
    p = Prog()
    p.layer(0, 0, WA[2], 2, 0, WA[1], da[1], A[2][0], None, save=(0, GTAPE["a2"][0]), aux=(1, TAPE["a2"][0]), transposed=True)
    p.layer(2, 0, WA[1], 1, 0, WA[0], da[0], A[1][0], None, save=(0, GTAPE["a1"][0]), aux=(1, TAPE["a1"][0]), transposed=True)
    p.layer(1, 0, WA[0], 2, 0, 57, 0, A[0][0], None, save=(0, GTAPE["ain"][0]), transposed=True)
    p.load((2, 1), 3, 4, WB[2])
    p.load((3, 1), 1, 0, WB[2])
    p.grad(1, 0, 3, 4, WB[2], add=True, save=(0, GTAPE["gb"][0]))
    p.layer(3, 4, WB[2], 1, 0, WB[1], db[1], B[2][0], None, save=(0, GTAPE["b2"][0]), aux=(1, TAPE["b2"][0]), transposed=True)
    p.layer(1, 0, WB[1], 3, 0, WB[0], db[0], B[1][0], None, save=(0, GTAPE["b1"][0]), aux=(1, TAPE["b1"][0]), transposed=True)
    p.layer(3, 0, WB[0], 1, 0, 61, 0, B[0][0], None, save=(0, GTAPE["bin"][0]), transposed=True)
    return Case("two-strand input-gradient chain", "composite", p, x, {1: tape, 2: g1, 3: g2}, {0: GTAPE["bin"][0] + 61}, "plain")


ACT0 = _act0_table()
LAYER_CASES = ACT0 + _act_table()
ELEMENTWISE = _elementwise_table()
_ids = lambda cases: [c.tag for c in cases]


# ------------------------------------------------------------------------------------------------------------------------ running a case
def _host_inputs(case):
    """-> x view (rows, x_cols) in the case's layout, outputs {slot: int32 array (rows + 16, stride)} holding the sentinel (written slots) or the
    supplied tensor in its first columns"""
    rows, xc = case.rows, case.x_cols
    if case.layout == "strided":
        x = np.full((rows, xc + 7), POISON, np.float32)[:, :xc]
    elif case.layout == "misaligned":
        x = np.zeros(rows * (xc + 2) + 1, np.float32)[1:].reshape(rows, xc + 2)[:, :xc]
    else:
        x = np.zeros((rows, xc), np.float32)
    x[...] = case.x
    outs = {}
    for slot in sorted(set(case.widths) | set(case.supplied)):
        width = max(case.widths.get(slot, 0), case.supplied[slot].shape[1] if slot in case.supplied else 0)
        a = np.full((rows + 16, width + 5), SENTINEL, np.int32)
        if slot in case.supplied:
            a[:rows, :case.supplied[slot].shape[1]] = case.supplied[slot].view(np.int32)
        outs[slot] = a
    return x, outs


def _judge(case, before, after, who):
    """every written element within the carried bound of the float64 value (a bound of zero: equal); everything else bit-identical to what was there
    -> the largest err / bound"""
    worst = 0.0
    for slot, r in case.reference.items():
        w = np.zeros(before[slot].shape, bool)
        w[:case.rows, :r.written.shape[1]] = r.written
        assert np.array_equal(after[slot][~w], before[slot][~w]), f"{who}: {case.tag}: slot {slot} changed outside what the program writes"
        if not r.written.any():
            continue
        got = after[slot].view(np.float32)[:case.rows, :r.written.shape[1]].astype(np.float64)
        err = np.abs(got - r.val)[r.written]
        bound = r.err[r.written]
        assert np.isfinite(bound).all()
        ok = err <= bound                                # (a NaN is not <= anything; a bound of zero asks for the very value)
        pos = bound > 0
        ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
        print("MEASURED", who, case.group, "|", case.tag, "| slot %d max_err=%.3e bound_there=%.3e err/bound=%.3f" % (
            slot, float(np.nanmax(err)) if err.size else 0.0, float(bound[np.nanargmax(err)]) if err.size else 0.0, ratio))
        assert ok.all(), f"{who}: {case.tag}: slot {slot}: {int((~ok).sum())} of {ok.size} outside the bound, worst err {np.nanmax(np.where(ok, 0, err)):.3e}"
        worst = max(worst, ratio)
    return worst


def _slot_tables(outs, ptr):
    k = max(outs) + 1 if outs else 0
    ptrs = (C.c_void_p * max(k, 1))(*[ptr(outs[s]) if s in outs else None for s in range(k)])
    strides = (C.c_int64 * max(k, 1))(*[(outs[s].shape[1] if s in outs else 0) for s in range(k)])
    return ptrs, strides, k


def run_twin(case):
    lib = load_oracle()
    p = case.prog
    x, outs = _host_inputs(case)
    before = {s: a.copy() for s, a in outs.items()}
    ops = p.c_ops()
    packed = np.zeros(max(p.end, 4), np.float32)
    w = (C.c_void_p * p.n)(*[(a.ctypes.data if a is not None else None) for a in p.w])
    b = (C.c_void_p * p.n)(*[(a.ctypes.data if a is not None else None) for a in p.b])
    if any(a is not None for a in p.w):
        assert lib.qo_mlp_pack(ops, p.n, w, b, packed.ctypes.data, packed.size, None) == 0
    ptrs, strides, k = _slot_tables(outs, lambda a: a.ctypes.data)
    rc = lib.qo_mlp_forward(x.ctypes.data, x.strides[0] // 4, case.rows, case.x_cols, ops, p.n, packed.ctypes.data, ptrs, strides, k, None)
    assert rc == 0, (case.tag, rc)
    return _judge(case, before, outs, "twin")


def launch_gpu(case, x_dev=None):
    """-> ({slot: int32 array before}, {slot: int32 array after}) of one qa_mlp_pack + qa_mlp_forward"""
    import torch
    lib = qa()
    p = case.prog
    x, outs = _host_inputs(case)
    # the same layout on the device: the view's offset and strides are kept
    base = x.base if x.base is not None else x
    while base.base is not None:
        base = base.base
    flat = torch.from_numpy(np.ascontiguousarray(base).reshape(-1)).cuda()
    xd = torch.as_strided(flat, x.shape, [s // 4 for s in x.strides], (x.ctypes.data - base.ctypes.data) // 4)
    assert xd.data_ptr() % 16 != 0 or case.layout != "misaligned"
    od = {s: torch.from_numpy(a).cuda() for s, a in outs.items()}
    wd = [None if a is None else torch.from_numpy(a).cuda() for a in p.w]
    bd = [None if a is None else torch.from_numpy(a).cuda() for a in p.b]
    packed = torch.zeros(max(p.end, 4), dtype=torch.float32, device="cuda")
    ops = p.c_ops()
    w = (C.c_void_p * p.n)(*[(t.data_ptr() if t is not None else None) for t in wd])
    b = (C.c_void_p * p.n)(*[(t.data_ptr() if t is not None else None) for t in bd])
    api = _capi.API
    assert lib.qa_mlp_packed_floats(ops, p.n) == p.end
    api.launch("mlp_pack", ops, p.n, w, b, C.c_void_p(packed.data_ptr()), packed.numel(), on=packed)
    ptrs, strides, k = _slot_tables(od, lambda t: t.data_ptr())
    for s, t in od.items():
        strides[s] = t.stride(0)
    api.launch("mlp_forward", C.c_void_p(xd.data_ptr()), xd.stride(0), case.rows, case.x_cols, ops, p.n, C.c_void_p(packed.data_ptr()), ptrs, strides, k, on=xd)
    torch.cuda.synchronize()
    return outs, {s: t.cpu().numpy() for s, t in od.items()}


def run_gpu(case):
    before, after = launch_gpu(case)
    return _judge(case, before, after, "hip"), after


# ------------------------------------------------------------------------------------------------------------------------ CPU
def _two_group_plan_applies(case):
    n = case.prog.n
    plan = [(C.c_int32 * n)(), (C.c_int32 * 8)(), (C.c_int32 * 8)(), (C.c_int32 * 1)()]
    assert qa().qa_mlp_groups(case.prog.c_ops(), n, case.x_cols, *plan) == 1, "the two-group launch does not apply"
    assert sorted(-(-((op.n + 15) // 16) // 4) for op in case.prog.ops if (op.n + 15) // 16 > 1) == [1, 2, 4, 8]


def test_composites_are_what_the_gpu_tests_need():
    _two_group_plan_applies(composite_forward())
    for case in (composite_forward(), composite_forward(True), composite_backward()):
        assert _strands(qa(), "qa_", case.prog.c_ops(), case.prog.n)[0] == 2, case.tag
        assert _strands(load_oracle(), "qo_", case.prog.c_ops(), case.prog.n) == _strands(qa(), "qa_", case.prog.c_ops(), case.prog.n)


def test_case_tables_cover_what_they_claim():
    ks, ns = {}, {}
    for c in ACT0:
        ks.setdefault(c.meta["k"], set()).add(c.meta["n"]); ns.setdefault(c.meta["n"], set()).add(c.meta["k"])
    assert set(ks) == set(K_SET) and set(ns) == set(N_SET) and len(LAYER_CASES) <= 40
    assert all(len(v) >= 2 for v in ks.values()) and all(len(v) >= 2 for v in ns.values()), (ks, ns)
    for key, want in (("scol", {0, 4, 36}), ("dcol", {0, 1, 3, 13}), ("ocol", {0, 1, 3, 13}), ("mode", {"A", "B"}), ("bias", {True, False})):
        assert {c.meta[key] for c in ACT0} == want, key
    assert any(c.meta["scol"] + c.meta["k"] == COLS[0] + 4 for c in ACT0)
    assert {c.rows for c in LAYER_CASES} == set(ROWS) and {c.layout for c in LAYER_CASES} == set(LAYOUTS)
    assert any(c.x_cols == 671 for c in ACT0)
    assert sorted(c.meta["act"] for c in LAYER_CASES if c.meta["act"]) == [1, 2, 3] + list(range(4, 13))
    for c in LAYER_CASES:
        if c.meta["act"] in ref.GRAD_CODES:
            y = c.supplied[2][:, 3:]
            assert (y == 0).any() and (y > 0).any() and (y < 0).any(), c.tag
    assert all(c.prog.n <= _capi.MLP_MAX_OPS for c in LAYER_CASES + ELEMENTWISE)


@pytest.mark.parametrize("case", LAYER_CASES + ELEMENTWISE, ids=_ids(LAYER_CASES + ELEMENTWISE))
def test_twin_equals_interpreter(case):
    run_twin(case)


@pytest.mark.parametrize("rows", [33, COMPOSITE_ROWS])
def test_twin_equals_interpreter_on_the_composites(rows):
    for case in (composite_forward(), composite_forward(True), composite_backward()):
        run_twin(case.with_rows(rows))


@pytest.mark.parametrize("case", ACT0, ids=_ids(ACT0))
def test_act0_bounds_have_teeth(case):
    """from the reference alone: every product term is >= 0.25 and the bound is <= 802 * 2^-24 * 800, so a reference with one k element zeroed, and
    one with a 16-column tile of the result shifted by a column, must both fall outside the bound"""
    m = case.meta
    r = case.reference[0]
    cols = slice(m["ocol"], m["ocol"] + m["n"])
    val, err = r.val[:, cols], r.err[:, cols]
    assert r.written[:, cols].all() and err.max() <= 802 * 2.0 ** -24 * 800 < 0.25
    live = min(m["k"], case.x_cols - m["x_live_col"])
    assert np.abs(case.x[:, m["x_live_col"]:m["x_live_col"] + live]).min() >= 0.5 and np.abs(case.prog.w[-2 if m["mode"] == "B" else -1]).min() >= 0.5
    x2 = case.x.copy()
    x2[:, m["x_live_col"] + live // 2] = 0.0
    dropped = ref.run(case.prog.ops, case.prog.w, case.prog.b, x2, case.x_cols, case.supplied, case.widths)[0].val[:, cols]
    assert (np.abs(dropped - val) > err).all(), case.tag
    if m["n"] > 1:                                      # (a single column has nowhere to shift to: misplacing it is the sentinel's business)
        t0 = ((m["n"] + 15) // 16 - 1) // 2 * 16
        t1 = min(t0 + 16, m["n"])
        shifted = val.copy()
        shifted[:, t0:t1] = np.roll(val[:, t0:t1], 1, axis=1)
        assert (np.abs(shifted - val) > err).any(), case.tag


def _strands(lib, prefix, ops, n):
    out = (C.c_int32 * n)()
    return getattr(lib, prefix + "mlp_strands")(ops, n, 4, out), list(out)


def _layer(**kw):
    d = dict(kind=ref.LAYER, src_buf=0, src_col=0, dst_buf=1, dst_col=0, k=16, n=16)
    d.update(kw)
    return _capi.QaMlpOp(**d)


REFUSALS = {
    "n = 513": ([_layer(n=513, dst_buf=-1)], False),
    "src_col % 4 != 0": ([_layer(src_col=2)], False),
    "a layer's dst_buf == src_buf": ([_layer(src_buf=1, dst_buf=1, dst_col=64)], True),
    "overlapping COPY ranges in one buffer": ([_capi.QaMlpOp(kind=ref.COPY, src_buf=1, src_col=0, dst_buf=1, dst_col=8, n=16)], False),
    "a LOAD into buffer 0": ([_capi.QaMlpOp(kind=ref.LOAD, dst_buf=0, n=4)], True),
    "an unknown flag bit": ([_layer(flags=8)], False),
    "w_off % 4 != 0": ([_layer(w_off=2)], False),
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusals(what):
    """qa_mlp_strands runs the library's whole validation on the host; where the twin has the same check it refuses too"""
    ops, twin_too = REFUSALS[what]
    c_ops = (_capi.QaMlpOp * len(ops))(*ops)
    good = (_capi.QaMlpOp * 1)(_layer())
    assert _strands(qa(), "qa_", good, 1)[0] == 1, qa().qa_last_error().decode()
    assert _strands(qa(), "qa_", c_ops, len(ops))[0] == E_ARG, what
    if twin_too:
        lib = load_oracle()
        x, packed, out = np.zeros((1, 16), np.float32), np.zeros(1024, np.float32), np.zeros((1, 16), np.float32)
        ptrs, strides = (C.c_void_p * 1)(out.ctypes.data), (C.c_int64 * 1)(16)
        assert lib.qo_mlp_forward(x.ctypes.data, 16, 1, 16, good, 1, packed.ctypes.data, ptrs, strides, 1, None) == 0
        assert lib.qo_mlp_forward(x.ctypes.data, 16, 1, 16, c_ops, len(ops), packed.ctypes.data, ptrs, strides, 1, None) == E_ARG, what


def test_a_program_must_not_read_back_what_it_writes():
    """include/qa_sim.h, "global tensors within one launch": the strands of a tile are separate workgroups, so an op reading (aux, or LOAD) columns of
    outs[i] that an earlier op of the program writes is refused -- by the library and by the twin; disjoint columns and other slots are fine"""
    def programs(col, slot):
        save = Prog().copy(0, 0, 1, 0, 8, save=(0, 4))
        yield "LOAD after SAVE", Prog().copy(0, 0, 1, 0, 8, save=(0, 4)).load((slot, col), 2, 0, 8)
        yield "saved activation after SAVE", save.grad(0, 0, 2, 0, 8, act=4, aux=(slot, col))
        w = np.ones((8, 16), np.float32)
        yield "epilogue after a layer's global output", Prog().layer(0, 0, 16, -1, 0, 8, 0, w, None, out=(0, 4)).layer(0, 0, 16, 1, 0, 8, 6, w.T.copy(), None, aux=(slot, col), transposed=True)
    qo = load_oracle()
    for col, slot, ok in ((4, 0, False), (11, 0, False), (0, 0, False), (12, 0, True), (4, 1, True)):
        for name, p in programs(col, slot):
            ns = _strands(qa(), "qa_", p.c_ops(), p.n)[0]
            assert (ns >= 1) == ok and (ok or ns == E_ARG), (name, col, slot, ns)
            assert (_strands(qo, "qo_", p.c_ops(), p.n)[0] >= 1) == ok, (name, col, slot)
    # the other order (read, then written) is a program like any other
    p = Prog().load((0, 4), 2, 0, 8).copy(0, 0, 1, 0, 8, save=(0, 4))
    assert _strands(qa(), "qa_", p.c_ops(), p.n)[0] >= 1 and _strands(qo, "qo_", p.c_ops(), p.n)[0] >= 1


def test_every_shipped_training_program_is_accepted_and_the_packers_joint_list_is_not_a_program():
    """the rule above is about ONE launch: each program the three training chains describe passes the library's own validation (qa_mlp_strands,
    host-only), while the op list their packer hands qa_mlp_pack -- the layers of a step's programs side by side, one program writing the tape slot
    the next one reads -- is no program to run: qa_mlp_pack must not apply the rule to it (it did once, and every chain step failed to pack)"""
    from quadrupedal_agility_amd.rsl_rl.algorithms import mlp_program, train_chain
    from tests.test_policy_chain import tsc_modules
    from tests.test_train_chain import _disc, _modules
    lib = load_oracle()
    ac, est, _ = _modules()
    tac, test_, _ = tsc_modules(4)
    chains = [train_chain.PpoTrainChain.describe(ac, est, 37, lib=lib, prefix="qo_"), train_chain.DiscTrainChain.describe(_disc(), 69, 23, lib=lib, prefix="qo_"),
              train_chain.TscTrainChain.describe(tac, test_, 21, 57, lib=lib, prefix="qo_")]
    crossing = 0
    for chain in chains:
        assert chain is not None
        for prog in [v for v in vars(chain).values() if isinstance(v, mlp_program.Program)]:
            ns, _ = _strands(qa(), "qa_", prog.c_ops, prog.n_ops)
            assert ns >= 1, qa().qa_last_error().decode()
            assert _strands(lib, "qo_", prog.c_ops, prog.n_ops)[0] == ns
        for ops, n, _, _ in chain._packer.calls:
            crossing += _strands(qa(), "qa_", ops, n)[0] == E_ARG and b"of the same program writes" in qa().qa_last_error()
            assert lib.qo_mlp_packed_floats(ops, n) == qa().qa_mlp_packed_floats(ops, n) > 0
    assert crossing >= 1                                # the joint lists do look like that to the rule: the reason it stays out of qa_mlp_pack


@pytest.mark.gpu
def test_hip_pack_takes_the_layers_of_several_programs():
    """qa_mlp_pack on a joint list in which a later op's saved activation is a slot an earlier op writes (two programs' layers): packed, and each
    layer's weights land where its own program expects them"""
    import torch
    w1, w2 = np.ones((8, 16), np.float32), np.full((16, 8), 2.0, np.float32)
    joint = Prog().layer(0, 0, 16, -1, 0, 8, 0, w1, None, out=(0, 0)).layer(0, 0, 16, 1, 0, 8, 6, w2, None, aux=(0, 0), transposed=True)
    assert _strands(qa(), "qa_", joint.c_ops(), 2)[0] == E_ARG
    wd = [torch.from_numpy(a).cuda() for a in joint.w]
    packed = torch.zeros(joint.end, device="cuda")
    _capi.API.launch("mlp_pack", joint.c_ops(), 2, (C.c_void_p * 2)(*[t.data_ptr() for t in wd]), (C.c_void_p * 2)(None, None), C.c_void_p(packed.data_ptr()),
                     packed.numel(), on=packed)
    torch.cuda.synchronize()
    got = packed.cpu().numpy()
    o1, o2 = joint.ops
    assert set(np.unique(got[o1.w_off:o1.b_off])) == {0.0, 1.0} and set(np.unique(got[o2.w_off:o2.b_off])) == {0.0, 2.0}
    assert (got[o1.w_off:o1.b_off] == 1.0).sum() == 8 * 16 and (got[o2.w_off:o2.b_off] == 2.0).sum() == 8 * 16


# ------------------------------------------------------------------------------------------------------------------------ GPU
_worst = {}


def _record(group, ratio):
    _worst[group] = max(_worst.get(group, 0.0), ratio)
    print("MEASURED worst err/bound so far,", group, "= %.3f" % _worst[group])


@pytest.mark.gpu
@pytest.mark.parametrize("case", LAYER_CASES, ids=_ids(LAYER_CASES))
def test_hip_single_layers(case):
    _record(case.group, run_gpu(case)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ELEMENTWISE, ids=_ids(ELEMENTWISE))
def test_hip_elementwise(case):
    _record(case.group, run_gpu(case)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["forward", "forward with saves", "backward"])
def test_hip_composites_split_equals_unsplit(which):
    """against the interpreter at 2049 rows (129 tiles: one workgroup per tile) and at 1, 17 and 33 rows (strands in separate workgroups), and the few-row
    launches bit for bit against the same rows of the 2049-row launch"""
    full = {"forward": composite_forward, "forward with saves": lambda: composite_forward(True), "backward": composite_backward}[which]()
    ratio, big = run_gpu(full)
    _record("composite", ratio)
    ns = _strands(qa(), "qa_", full.prog.c_ops(), full.prog.n)[0]
    assert ns == 2, ns
    for rows in (1, 17, 33):
        part = full.with_rows(rows)
        ratio, small = run_gpu(part)
        _record("composite", ratio)
        for slot in full.widths:
            assert np.array_equal(small[slot][:rows], big[slot][:rows]), (which, rows, slot)


@pytest.mark.gpu
def test_hip_two_group_launch_is_bit_identical():
    """qa_mlp_set_groups(2) at 2049 rows: the forward chain's layers have 29, 13, 7 and 3 column tiles, so the group kernel takes all four of its
    tiles-per-wave branches (8, 4, 2, 1)"""
    case = composite_forward()
    lib = qa()
    n = case.prog.n
    _two_group_plan_applies(case)
    _, one = run_gpu(case)
    prev = lib.qa_mlp_set_groups(2)
    try:
        ratio, two = run_gpu(case)
    finally:
        lib.qa_mlp_set_groups(prev)
    _record("composite", ratio)
    for slot in case.widths:
        assert np.array_equal(one[slot], two[slot]), slot


@pytest.mark.gpu
def test_hip_forward_refuses_an_output_that_is_too_narrow():
    import torch
    lib = qa()
    p = Prog().layer(0, 0, 16, -1, 0, 16, 0, np.ones((16, 16), np.float32), None, out=(0, 3))
    x = torch.zeros(4, 16, device="cuda")
    packed = torch.zeros(p.end, device="cuda")
    out = torch.zeros(4, 19, device="cuda")
    ptrs = (C.c_void_p * 1)(out.data_ptr())
    call = lambda stride: lib.qa_mlp_forward(C.c_void_p(x.data_ptr()), 16, 4, 16, p.c_ops(), 1, C.c_void_p(packed.data_ptr()), ptrs, (C.c_int64 * 1)(stride), 1,
                                             _capi.stream(x))
    assert call(18) == E_ARG and b"too narrow" in lib.qa_last_error()
    assert call(19) == 0
    torch.cuda.synchronize()
