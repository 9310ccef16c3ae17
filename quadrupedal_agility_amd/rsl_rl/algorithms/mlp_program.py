"""The one builder of programs for `qa_mlp_forward` (include/qa_sim.h): a list of `QaMlpOp` (copy / load / grad / layer) over the kernel's four
LDS buffers plus the packed weight buffer whose offsets the list fixes.  fused.PolicyChain writes the rollouts' programs with it, train_chain the
training steps'.  Every op is held to the kernel's own rule (`mlp_check`, csrc/qa_policy.hip) where it is added: `Misfit` says the modules do not
fit the kernel, before any launch."""
import ctypes as C

import torch

from quadrupedal_agility_amd import _capi
from quadrupedal_agility_amd._capi import _ptr

COLS = _capi.MLP_BUF_COLS
LDS_FLOATS = sum(16 * (c + 4) for c in COLS)          # a 16-row tile of every buffer, each row padded by 4
MAX_TILES = 32                                        # 16-wide column tiles of one layer: 4 per wave (4 * MLP_WAVES)


class Misfit(Exception):
    """an op the kernel's rule does not admit, or more ops than a program holds"""


def k_blocks(k, n):
    """16-wide k-blocks a layer is stored with (qa_policy.hip mlp_kb): rounded up to the kernel's prefetch depth"""
    per = ((n + 15) // 16 + 7) // 8
    pf = 4 if per > 2 else 8
    return ((k + 15) // 16 + pf - 1) // pf * pf


def _need(ok, *what):
    if not ok:
        raise Misfit(what)


def out_tables(outs):
    """(pointers, row strides, count) of a launch's global tensors, as qa_mlp_forward takes them"""
    k = len(outs)
    return (C.c_void_p * k)(*[o.data_ptr() for o in outs]), (C.c_int64 * k)(*[o.stride(0) for o in outs]), k


class Program:
    """an op list + its packed weights.  A layer's (weight, bias) are tensors, or callables that build them when the weights are packed (the
    history encoder's structured matrices)."""

    def __init__(self, lib=None, prefix="qa_"):
        self.ops, self.params, self.woff = [], [], 0
        self.packed = None
        self.api = _capi.Api(lib, prefix)          # injection point of the tests (another library exporting the same entry points under another prefix); the default is libqa_sim.so, and it is required

    def _add(self, op, param):
        self.ops.append(op); self.params.append(param)

    # ---- the ops.  Each mirrors its clause of mlp_check (csrc/qa_policy.hip): what passes here, the library accepts
    @staticmethod
    def _into(dst, dcol, n):
        return n > 0 and 0 < dst < len(COLS) and dcol >= 0 and dcol + n <= COLS[dst]

    @classmethod
    def _moves(cls, src, scol, dst, dcol, n):
        return (cls._into(dst, dcol, n) and 0 <= src < len(COLS) and scol >= 0 and scol + n <= COLS[src]
                and (dst != src or dcol >= scol + n or scol >= dcol + n))

    def copy(self, src, scol, dst, dcol, n, save=None):
        _need(self._moves(src, scol, dst, dcol, n), "copy", src, scol, dst, dcol, n)
        kw = dict(flags=_capi.MLP_F_SAVE, out_index=save[0], out_col=save[1]) if save else {}
        self._add(_capi.QaMlpOp(kind=_capi.MLP_COPY, src_buf=src, src_col=scol, dst_buf=dst, dst_col=dcol, k=0, n=n, **kw), None)

    def load(self, aux, dst, dcol, n, save=None):
        """scratch buffer <- columns of a global tensor (aux = (output slot, first column))"""
        _need(self._into(dst, dcol, n), "load", dst, dcol, n)
        kw = dict(flags=_capi.MLP_F_SAVE, out_index=save[0], out_col=save[1]) if save else {}
        self._add(_capi.QaMlpOp(kind=_capi.MLP_LOAD, src_buf=0, src_col=0, dst_buf=dst, dst_col=dcol, k=0, n=n, aux_index=aux[0], aux_col=aux[1], **kw), None)

    def grad(self, src, scol, dst, dcol, n, act=0, aux=None, add=False, save=None):
        _need(self._moves(src, scol, dst, dcol, n), "grad", src, scol, dst, dcol, n)
        flags = (_capi.MLP_F_ADD if add else 0) | (_capi.MLP_F_SAVE if save else 0)
        kw = dict(out_index=save[0], out_col=save[1]) if save else {}
        if aux:
            kw.update(aux_index=aux[0], aux_col=aux[1])
        self._add(_capi.QaMlpOp(kind=_capi.MLP_GRAD, src_buf=src, src_col=scol, dst_buf=dst, dst_col=dcol, k=0, n=n, act=act, flags=flags, **kw), None)

    def layer(self, src, scol, k, dst, dcol, n, act, weight, bias, out=None, save=None, aux=None, transposed=False):
        """dst >= 0: into scratch buffer dst (and, with `save` = (output, column), to that global output too); dst = -1: to `out` = (output, column)"""
        nt, kb = (n + 15) // 16, k_blocks(k, n)
        # mlp_check's layer clause.  The k-blocks beyond k are read against zero weights; they may run past the row's padding into the next row /
        # buffer, but not past the kernel's LDS
        _need(k > 0 and n > 0 and 0 <= src < len(COLS) and dst != src and scol >= 0 and scol % 4 == 0 and scol + k <= COLS[src] + 4
              and (dst < 0 or self._into(dst, dcol, n)) and nt <= MAX_TILES
              and sum(16 * (c + 4) for c in COLS[:src]) + 15 * (COLS[src] + 4) + scol + 16 * kb <= LDS_FLOATS, "layer", src, scol, k, dst, dcol, n)
        w_off = self.woff; b_off = w_off + nt * kb * 256; self.woff = b_off + nt * 16
        flags = (_capi.MLP_F_SAVE if (save and dst >= 0) else 0) | (_capi.MLP_F_TRANSPOSED if transposed else 0)
        oi, oc = (out if dst < 0 else save) or (0, 0)
        ai, acol = aux or (0, 0)
        self._add(_capi.QaMlpOp(kind=_capi.MLP_LAYER, src_buf=src, src_col=scol, dst_buf=dst, dst_col=dcol, k=k, n=n, act=act, out_index=oi, flags=flags,
                                w_off=w_off, b_off=b_off, out_col=oc, aux_index=ai, aux_col=acol), (weight, bias))

    def stack(self, layers, src, scol, k, final, reserved=()):
        """[(Linear, act code)] one after the other through the scratch buffers, from columns scol.. of buffer src; the last one to `final` =
        ("buf", b, col) or ("out", index), every other to the first of buffers 3, 2, 1 that is neither its source nor `reserved` and wide enough"""
        for i, (lin, act) in enumerate(layers):
            n = lin.out_features
            _need(lin.in_features == k, "stack", i, lin.in_features, k)
            if i == len(layers) - 1:
                dst, dcol, out = (final[1], final[2], None) if final[0] == "buf" else (-1, 0, (final[1], 0))
            else:
                fit = [b for b in (3, 2, 1) if b != src and b not in reserved and COLS[b] >= n]
                _need(fit, "stack", i, n)
                dst, dcol, out = fit[0], 0, None
            self.layer(src, scol, k, dst, dcol, n, act, lin.weight, lin.bias, out=out)
            src, scol, k = dst, 0, n

    # ---- the finished list, its weights and its launches
    def seal(self):
        """the op list is complete: its ctypes form"""
        _need(0 < len(self.ops) <= _capi.MLP_MAX_OPS, "ops", len(self.ops))
        self.n_ops = len(self.ops)
        self.c_ops = (_capi.QaMlpOp * self.n_ops)(*self.ops)
        return self

    def ptr_arrays(self):
        """pointers of every layer's (weight, bias), for qa_mlp_pack; parameters that are callables are built here, and what they built stays
        referenced in self.built"""
        self.built = [tuple((t() if callable(t) else t) for t in p) if p else None for p in self.params]
        w = (C.c_void_p * self.n_ops)(*[(p[0].data_ptr() if p else None) for p in self.built])
        b = (C.c_void_p * self.n_ops)(*[(p[1].data_ptr() if p and p[1] is not None else None) for p in self.built])
        return w, b

    def bind(self):
        """the weights as they are now -> the pointer tables `pack()` hands over; allocates the packed buffer the first time"""
        self.w_ptrs, self.b_ptrs = self.ptr_arrays()
        for p in self.built:
            if p and not ((p[0].is_cuda or self.api.prefix != "qa_") and p[0].is_contiguous() and p[0].dtype == torch.float32):
                raise RuntimeError("chain program: parameters must be contiguous fp32 ROCm tensors")
        if self.packed is None:
            self.packed = torch.zeros(self.woff, dtype=torch.float32, device=next(p[0] for p in self.built if p).device)

    def finish(self):
        self.seal().bind()

    def pack(self):
        self.api.launch("mlp_pack", self.c_ops, self.n_ops, self.w_ptrs, self.b_ptrs, _ptr(self.packed), self.woff, on=self.packed)

    def launch(self, x, x_cols, outs=None, tables=None):
        """`outs`: the launch's global tensors; or `tables` = out_tables(outs), built once by a caller that keeps its tensors"""
        ptrs, strides, k = tables or out_tables(outs)
        self.api.launch("mlp_forward", _ptr(x), x.stride(0), x.shape[0], x_cols, self.c_ops, self.n_ops, _ptr(self.packed), ptrs, strides, k, on=x)


class Packer:
    """qa_mlp_pack for SEVERAL programs in one launch: their layers as one op list over one packed buffer (each program's `packed` becomes its slice).
    The weights change with every optimiser step, so a chain step repacks before it runs: one launch instead of one per program."""

    def __init__(self, programs):
        p0 = programs[0]
        self.prog = p0
        total = sum(p.woff for p in programs)
        self.buf = torch.zeros(total, dtype=torch.float32, device=p0.packed.device)
        ops, w, b, off = [], [], [], 0
        for p in programs:
            p.packed = self.buf[off:off + p.woff]
            for op, param in zip(p.ops, p.built):
                if op.kind == _capi.MLP_LAYER:
                    o2 = _capi.QaMlpOp.from_buffer_copy(op)
                    o2.w_off += off; o2.b_off += off
                    ops.append(o2); w.append(param[0].data_ptr()); b.append(param[1].data_ptr() if param[1] is not None else None)
            off += p.woff
        assert off == total
        M = _capi.MLP_MAX_OPS            # (a pack call takes at most this many layers: the task-level step's 30 go in two)
        self.calls = [((_capi.QaMlpOp * len(ops[i:i + M]))(*ops[i:i + M]), len(ops[i:i + M]), (C.c_void_p * len(ops[i:i + M]))(*w[i:i + M]),
                       (C.c_void_p * len(ops[i:i + M]))(*b[i:i + M])) for i in range(0, len(ops), M)]
        self.total = total

    def pack(self):
        for ops, n, w, b in self.calls:
            self.prog.api.launch("mlp_pack", ops, n, w, b, _ptr(self.buf), self.total, on=self.buf)
