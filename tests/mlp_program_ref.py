"""A float64 interpreter of qa_mlp_op programs, written from the contract of include/qa_sim.h ("Policy inference", the ABI 13 / 17 / 18 paragraphs) and
from nothing else: four buffers of QA_MLP_BUFn_COLS + 4 columns, zero at the start; buffer 0 takes x[:, :x_cols]; the ops run in order; weights are
taken unpacked, as nn.Linear stores them (for QA_MLP_F_TRANSPOSED: the forward layer's matrix).  No tiles, no packing, no strands.

Beside every value it carries an ABSOLUTE bound on |what an fp32 evaluation of the same program may give - the float64 value| (a running error
analysis, u = 2^-24):
  LAYER   e = L_act * ((k + 2) u (|x| @ |W|^T + |b|) + e_in @ |W|^T) + e_act.  The first term bounds an fp32 dot product of k terms plus a bias in ANY
          summation order; the second carries the inputs' own bounds through the (linear) product; L_act is the activation's Lipschitz constant
          (1; lambda alpha for SELU; 1/4 for sigmoid).
  e_act   the project's 3 x rule (tests/parity_tol.py, test_activations.py::_allow): 3 x the largest error of torch's own fp32 activation against
          float64 on that op's pre-activations; for ELU at least 2^-22, the relative error qa_policy.hip states for __expf (of e^v <= 1).  Zero for act 0.
  COPY / LOAD   carry the bound; a tensor the caller supplies has bound 0.
  derivative factors (act 4..6, 10..12, in a layer's epilogue or a GRAD op): v = p * d(y) with y exact (a supplied fp32 tensor), so
          e' = |d| e_p + (|p| + e_p) e_d, e = e' + u (|p d| + e'): the product rule with the rounding of d (e_d, per code below), then the
          rounding of the product that was formed.
  GRAD with ADD   e' = e_src + e_dst, e = e' + u (|src + dst| + e') before the factor.
Test infrastructure only (numpy for the arithmetic; torch only for e_act)."""
import numpy as np

U = 2.0 ** -24
BUF_COLS = (800, 576, 320, 128)                      # QA_MLP_BUFn_COLS
COPY, LAYER, GRAD, LOAD = 0, 1, 2, 3
F_SAVE, F_TRANSPOSED, F_ADD = 1, 2, 4
SELU_LAMBDA, SELU_ALPHA = 1.0507009873554805, 1.6732632423543772
FORWARD_CODES, GRAD_CODES = (0, 1, 2, 3, 7, 8, 9), (4, 5, 6, 10, 11, 12)
LIPSCHITZ = {0: 1.0, 1: 1.0, 2: 1.0, 3: 1.0, 7: 1.0, 8: SELU_LAMBDA * SELU_ALPHA, 9: 0.25}


def forward64(code, v):
    """act 0..3, 7..9 as the header writes them"""
    if code == 0:
        return v
    if code == 1:
        return np.where(v > 0, v, np.expm1(np.minimum(v, 0)))
    if code == 2:
        return np.maximum(v, 0.0)
    if code == 3:
        return np.tanh(v)
    if code == 7:
        return np.where(v > 0, v, 0.01 * v)
    if code == 8:
        return SELU_LAMBDA * np.where(v > 0, v, SELU_ALPHA * np.expm1(np.minimum(v, 0)))
    if code == 9:
        return 1.0 / (1.0 + np.exp(-v))
    raise ValueError(code)


def derivative64(code, y):
    """act 4..6, 10..12: the derivative from the saved OUTPUT y, exactly as the header writes it -> (d, e_d).  e_d bounds what fp32 loses evaluating d
    from the exact fp32 y: one rounding per operation, over the magnitudes of the terms; the constants 0.01, lambda and lambda alpha are fp32 too
    (lambda alpha is a rounded product of two rounded constants: 3 u)."""
    if code == 4:
        return np.where(y > 0, 1.0, y + 1.0), np.where(y > 0, 0.0, U * (np.abs(y) + 1.0))
    if code == 5:
        return np.where(y > 0, 1.0, 0.0), np.zeros_like(y)
    if code == 6:
        return 1.0 - y * y, U * (y * y) + U * (1.0 + y * y)
    if code == 10:
        return np.where(y > 0, 1.0, 0.01), np.where(y > 0, 0.0, U * 0.01)
    if code == 11:
        la = SELU_LAMBDA * SELU_ALPHA
        return np.where(y > 0, SELU_LAMBDA, y + la), np.where(y > 0, U * SELU_LAMBDA, 3 * U * la + U * (np.abs(y) + la))
    if code == 12:
        return y * (1.0 - y), U * np.abs(y) * (1.0 + np.abs(y)) + U * np.abs(y * (1.0 - y))
    raise ValueError(code)


def activation_error(code, pre):
    """e_act of the module docstring, from the references alone: torch's fp32 activation on fp32(pre) against float64 on pre"""
    if code == 0:
        return 0.0
    import torch
    import torch.nn.functional as F
    fn = {1: F.elu, 2: F.relu, 3: torch.tanh, 7: lambda t: F.leaky_relu(t, 0.01), 8: F.selu, 9: torch.sigmoid}[code]
    own = fn(torch.from_numpy(np.ascontiguousarray(pre)).float()).double().numpy()
    e = 3.0 * float(np.abs(own - forward64(code, pre)).max())
    return max(e, 2.0 ** -22) if code == 1 else e


class _Tracked:
    """values and their bounds, side by side"""

    def __init__(self, rows, cols):
        self.v, self.e = np.zeros((rows, cols)), np.zeros((rows, cols))


class Output:
    """one global tensor after the program: val / err (rows, cols) float64, written (rows, cols) bool = the elements the program wrote"""

    def __init__(self, val, err, written):
        self.val, self.err, self.written = val, err, written


def run(ops, weights, biases, x, x_cols, supplied, widths):
    """ops: qa_mlp_op-like objects (the header's field names); weights[i] / biases[i]: float arrays as nn.Linear stores them, or None; x: (rows, >=
    x_cols) fp32; supplied: {slot: (rows, cols) fp32 array} = the global tensors the caller hands in (read as `aux` or by LOAD); widths: {slot: columns}
    of the tensors the program writes.  -> {slot: Output} for every slot of `supplied` and `widths`."""
    rows = x.shape[0]
    buf = [_Tracked(rows, c + 4) for c in BUF_COLS]
    assert 0 < x_cols <= BUF_COLS[0]
    buf[0].v[:, :x_cols] = np.asarray(x, np.float64)[:, :x_cols]
    glob, written = {}, {}
    for slot in set(supplied) | set(widths):
        cols = max(widths.get(slot, 0), supplied[slot].shape[1] if slot in supplied else 0)
        glob[slot] = _Tracked(rows, cols)
        written[slot] = np.zeros((rows, cols), bool)
        if slot in supplied:
            glob[slot].v[:, :supplied[slot].shape[1]] = np.asarray(supplied[slot], np.float64)

    def put(op, v, e):
        g = glob[op.out_index]
        g.v[:, op.out_col:op.out_col + op.n], g.e[:, op.out_col:op.out_col + op.n] = v, e
        written[op.out_index][:, op.out_col:op.out_col + op.n] = True

    def factor(op, p, ep):
        y = glob[op.aux_index].v[:, op.aux_col:op.aux_col + op.n]
        assert not glob[op.aux_index].e[:, op.aux_col:op.aux_col + op.n].any(), "the saved activation must be a supplied tensor"
        d, ed = derivative64(op.act, y)
        e = np.abs(d) * ep + (np.abs(p) + ep) * ed                     # of the exact product of the two fp32 factors
        return p * d, e + U * (np.abs(p * d) + e)                      # ... and its rounding

    for i, op in enumerate(ops):
        n = op.n
        if op.kind == LAYER:
            src = buf[op.src_buf]
            assert op.src_col + op.k <= BUF_COLS[op.src_buf] + 4 and (op.dst_buf < 0 or op.dst_col + n <= BUF_COLS[op.dst_buf])
            xs, es = src.v[:, op.src_col:op.src_col + op.k], src.e[:, op.src_col:op.src_col + op.k]
            w = np.asarray(weights[i], np.float64)
            w = w.reshape(op.k, n).T if op.flags & F_TRANSPOSED else w.reshape(n, op.k)
            b = np.zeros(n) if biases[i] is None else np.asarray(biases[i], np.float64).reshape(n)
            pre = xs @ w.T + b
            e = (op.k + 2) * U * (np.abs(xs) @ np.abs(w).T + np.abs(b)) + es @ np.abs(w).T
            if op.act in GRAD_CODES:
                v, e = factor(op, pre, e)
            else:
                v, e = forward64(op.act, pre), LIPSCHITZ[op.act] * e + activation_error(op.act, pre)
            if op.dst_buf >= 0:
                buf[op.dst_buf].v[:, op.dst_col:op.dst_col + n], buf[op.dst_buf].e[:, op.dst_col:op.dst_col + n] = v, e
            if op.dst_buf < 0 or op.flags & F_SAVE:
                put(op, v, e)
            continue
        dst = buf[op.dst_buf]
        assert op.dst_buf > 0 and op.dst_col + n <= BUF_COLS[op.dst_buf]
        if op.kind == LOAD:
            v, e = glob[op.aux_index].v[:, op.aux_col:op.aux_col + n].copy(), glob[op.aux_index].e[:, op.aux_col:op.aux_col + n].copy()
        else:
            assert op.kind in (COPY, GRAD) and op.src_col + n <= BUF_COLS[op.src_buf]
            v, e = buf[op.src_buf].v[:, op.src_col:op.src_col + n].copy(), buf[op.src_buf].e[:, op.src_col:op.src_col + n].copy()
        if op.kind == GRAD:
            if op.flags & F_ADD:
                v = v + dst.v[:, op.dst_col:op.dst_col + n]
                e = e + dst.e[:, op.dst_col:op.dst_col + n]
                e = e + U * (np.abs(v) + e)
            if op.act != 0:
                v, e = factor(op, v, e)
        dst.v[:, op.dst_col:op.dst_col + n], dst.e[:, op.dst_col:op.dst_col + n] = v, e
        if op.flags & F_SAVE:
            put(op, v, e)
    return {slot: Output(glob[slot].v, glob[slot].e, written[slot]) for slot in glob}
