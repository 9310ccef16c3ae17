"""The edge-case table of tests/gemm_ref.py through the oracle's C twins (qo_linear_forward / _backward_input / _backward_weight /
_backward_weight_batch / _forward_split), no GPU: the twins against float64 at the tile, tail and split edges the HIP kernels are tested at in
tests/test_gemm_edges.py -- and with them the harness itself: NaN-poisoned operands, sentinel-filled outputs and scratch, the ctypes calls,
the alignment classes.  The twins know the activations 0..2 only; the table's other activations run as ELU here.  Then the table against
itself: the restated plans give the splits, k-tile counts, workgroup totals and vector-width combinations each group is there for."""
from dataclasses import replace

import pytest
import torch

from tests import gemm_ref as R
from tests.oracle_lib import load_oracle


def _be():
    return R.Backend(load_oracle(), "qo_", "cpu")


def _twin(c):
    return c if c.act in R.TWIN_ACTS else replace(c, act=R.ACT_ELU)


# ---------------------------------------------------------------- the references and the harness against themselves
@pytest.mark.parametrize("act", R.ACTS)
def test_reference_activations_and_their_derivatives_from_the_output(act):
    """act_f64 against torch's own modules; dact_f64(y) against autograd's derivative at the pre-activation"""
    F = torch.nn.functional
    alpha = 0.7
    mod = {R.ACT_NONE: lambda v: v, R.ACT_ELU: lambda v: F.elu(v, alpha), R.ACT_RELU: torch.relu, R.ACT_TANH: torch.tanh, R.ACT_LRELU: F.leaky_relu,
           R.ACT_SELU: F.selu, R.ACT_SIGMOID: torch.sigmoid}[act]
    v = torch.linspace(-6, 6, 2401, dtype=torch.float64)
    v = v[v != 0].requires_grad_(True)
    y = mod(v)
    assert torch.allclose(R.act_f64(act, v.detach(), alpha), y.detach(), rtol=1e-12, atol=1e-14)
    y.sum().backward()
    assert torch.allclose(R.dact_f64(act, y.detach(), alpha), v.grad, rtol=1e-9, atol=1e-12)


def test_windows_poison_everything_else_and_catch_stray_writes():
    vals = torch.arange(15.0).view(3, 5)
    for cls, want_vec in (("a", 1), ("b", 1), ("c", 1), ("d", 1), ("e", 1)):
        w = R.Window(3, 5, cls, vals, "cpu")
        view = w.buf.as_strided((3, 5), (w.ld, 1), w.start)
        assert torch.equal(view, vals) and int(torch.isnan(w.buf).sum()) == w.size - 15 and w.vec(5) == want_vec
        assert w.start >= R.GUARD_ROWS * w.ld and w.size - (w.start + 2 * w.ld + 5) >= R.GUARD_ROWS * w.ld
    assert R.Window(3, 8, "a", torch.zeros(3, 8), "cpu").vec(8) == 4 and R.Window(3, 8, "d", torch.zeros(3, 8), "cpu").vec(8) == 4
    assert [R.Window(3, 8, c, torch.zeros(3, 8), "cpu").vec(8) for c in "bce"] == [1, 1, 1]
    out = R.Window(3, 5, "a", None, "cpu")
    with pytest.raises(AssertionError, match="not finite"):
        out.check("untouched")
    out.buf.as_strided((3, 5), (out.ld, 1), out.start).fill_(1.0)
    assert torch.equal(out.check("filled"), torch.ones(3, 5))
    out.buf[out.start + 5] = 2.0                                  # one element right of the first row
    with pytest.raises(AssertionError, match="outside the output window"):
        out.check("stray")
    s = R.Scratch(100, "cpu")
    s.check("untouched")
    s.buf[25] = 0.0                                               # the first float behind the declared 100 bytes
    with pytest.raises(AssertionError, match="behind the declared"):
        s.check("stray")


# ---------------------------------------------------------------- the table against the plans it is there for
def test_weight_gradient_rows_give_the_splits_they_are_there_for():
    for k, n in R.WGRAD_FEATURES:
        for cfg in (-1,) + R.CFGS:
            plans = [R.wgrad_plan(rows, k, n, cfg) for rows in R.WGRAD_ROWS]
            assert [p[1] for p in plans] == [1, 1, 1, 1, 1, 1, 1, 2, 3], (k, n, cfg)
            assert [p[2] for p in plans] == [16, 16, 16, 16, 32, 48, 48, 144, 176], (k, n, cfg)
    assert 257 - 144 == 113 and 513 - 2 * 176 == 161 and 113 % 16 == 1 and 161 % 16 == 1            # last splits end in a k-tile with one live row
    # five a-tiles against one k-tile under the 64-wide a-tiles: four of the five bias rows per split are written zeros
    for cfg in (2, 3, 13, 14):
        for rows in (1, 5, 15, 16):
            lay = R.wgrad_layout(rows, 300, 7, cfg)
            assert lay[0] == 1 and lay[2] == 5 and -(-rows // 16) == 1
    # a forced value that names no linear tile plans as 64 x 64, one outside every table as no force
    assert [R.resolve_forced(f) for f in (-1, 0, 3, 4, 9, 10, 14, 15, 99)] == [-1, 0, 3, 2, 2, 10, 14, -1, -1]
    assert R.wgrad_layout(40, 100, 12, 4) == R.wgrad_layout(40, 100, 12, 2) and R.wgrad_layout(40, 100, 12, 99) == R.wgrad_layout(40, 100, 12, -1)


def test_split_forward_shapes_give_the_splits_they_are_there_for():
    plans = [R.fwd_split_plan(*s) for s in R.SPLIT_SHAPES]
    assert plans == [(2, 272), (2, 256), (2, 304), (4, 272), (3, 256)]
    assert [k - (s - 1) * kps for (_, k, _), (s, kps) in zip(R.SPLIT_SHAPES, plans)] == [241, 256, 296, 224, 256]
    assert all(c.n % 4 == 0 and c.oc in "ad" and c.bc in ("a", None) for c in R.split_cases())
    assert R.fwd_split_plan(*R.SPLIT_SHAPE_DMA) == (2, 256) and [R.split_launch(c, (4, 4, 4), 13).dma for c in R.split_cases()[-1:]] == [True]


@pytest.mark.parametrize("product", ["forward", "backward_input"])
def test_layer_table_covers_the_edges_under_every_tile(product):
    for cfg in R.CFGS:
        g = R.layer_cases(product, cfg)
        ba, bb = R.tile_dims(cfg)
        launches = {name: [R.layer_launch(product, c, want, cfg) for c, want in cases if want] for name, cases in g.items()}
        assert sum(len(v) for v in g.values()) <= 70
        assert {want[:2] for _, want in g["vecs"]} == {(4, 4), (4, 1), (1, 4), (1, 1)}
        assert {want[2] for _, want in g["placement"]} == {1, 4}
        # o_vec == 4 with a width that is no multiple of 4: the scalar tail next to foreign data
        assert any(want[2] == 4 and (c.n if product == "forward" else c.k) % 4 for c, want in g["placement"])
        assert sorted(l.workgroups for l in launches["totals"]) == [1, 7, 8, 9, 15]
        assert all(l.dma == (cfg >= 10) and (l.ba, l.bb) == (ba, bb) for l in launches["totals"])
        assert all(l.dma == (cfg >= 10) for l in launches["dma_counts"]) and {want[2] for _, want in g["dma_counts"]} == {1, 4}
        assert sum(l.dma for l in launches["placement"]) == (0 if cfg < 10 else (6 if product == "forward" else 5))
        kt = sorted({-(-(c.k if product == "forward" else c.n) // 16) for c, _ in g["klens"]})
        assert kt == [1, 2, 3, 4]
        ring = launches["ring"]
        if cfg >= 10:
            assert [(l.dma, l.k_tiles) for l in ring] == [(True, 1), (True, 2), (True, 3), (True, 4), (False, 2)]
        else:
            assert not any(l.dma for l in ring)
        counts = R.COUNTS + (R.COUNTS_192 if bb == 192 else ())
        assert sorted((c.n if product == "forward" else c.k) for c, _ in g["counts"]) == sorted(counts) == sorted(c.rows for c, _ in g["counts"])
        assert {(c.k if product == "forward" else c.n) for c, _ in g["counts"]} | {(c.k if product == "forward" else c.n) for c, _ in g["klens"]} >= set(R.KLENS)
        assert all(c.rows <= 600 and c.k <= 1100 and c.n <= 1100 for cases in g.values() for c, _ in cases)


def test_weight_gradient_table_covers_every_vector_width_combination():
    got = {}
    for k, n in R.WGRAD_FEATURES:
        cases = R.wgrad_cases(k, n)
        assert [c.rows for c, _ in cases] == list(R.WGRAD_ROWS)
        got[(k, n)] = {want for _, want in cases}
        assert {c.oc for c, _ in cases} == {"d", "e"}
    assert all(got[f] == {(4, 4), (4, 1), (1, 4), (1, 1)} for f in ((100, 12), (64, 64), (132, 68)))
    assert got[(7, 3)] == {(1, 1)} and got[(300, 7)] == {(4, 1), (1, 1)}
    assert (7 * 3) % 4 != 0 and any(c.oc == "e" for c, _ in R.wgrad_cases(7, 3))                   # the scalar tail of the slab reduction at an unaligned address
    # the grouped launch: 14 of one class, all four classes in one call, the limit and one more
    flush = R.batch_cases("flush")
    assert len(flush) == 14 > 12 and all(c.xc == "a" and c.gc == "a" and c.k % 4 == 0 and c.n % 4 == 0 for c in flush)
    assert {R.wgrad_batch_plan(c.rows, c.k, c.n)[0] for c in flush} == {1, 2, 3}
    assert len(R.batch_cases("limit")) == 32 and len(R.batch_cases("over")) == 33
    assert any(c.rows == 5 for c in R.batch_cases("classes")) and any((c.rows, c.k, c.n) == (40, 130, 3) for c in R.batch_cases("classes"))


# ---------------------------------------------------------------- the twins over the table
def _check_layer(be, product, c, want):
    out = (R.run_forward if product == "forward" else R.run_backward_input)(be, _twin(c))
    if want:
        assert out.vec == want, (c, out.vec, want)
    kred = c.k if product == "forward" else c.n
    assert R.close(out.got, out.ref, **R.tol_layer(kred)), (product, c, R.worst(out.got, out.ref))


def _distinct_layer_cases(product):
    seen = {}
    for cfg in R.CFGS:
        for name, cases in R.layer_cases(product, cfg).items():
            for c, want in cases:
                seen.setdefault((name, c), want)
    return seen


@pytest.mark.parametrize("product", ["forward", "backward_input"])
def test_twin_layers_over_the_whole_table(product):
    be = _be()
    for (name, c), want in _distinct_layer_cases(product).items():
        _check_layer(be, product, c, want)
    for c, want in R.activation_cases(product):
        _check_layer(be, product, c, want)


def test_twin_split_forward():
    be = _be()
    for c in R.split_cases():
        one, two = R.run_forward_split(be, _twin(c))
        assert R.same_bits(one.got, two.got)
        assert R.close(one.got, one.ref, **R.tol_layer(c.k)), (c, R.worst(one.got, one.ref))


@pytest.mark.parametrize("k,n", R.WGRAD_FEATURES)
def test_twin_weight_gradient(k, n):
    be = _be()
    for c, want in R.wgrad_cases(k, n):
        fin = R.run_backward_weight(be, c, finished=True)
        par = R.run_backward_weight(be, c, finished=False)
        assert fin.vec[:2] == want == par.vec[:2], (c, fin.vec, want)
        tol = R.tol_wgrad(c.rows)
        assert R.close(fin.gw, fin.ref_w, **tol) and R.close(fin.gb, fin.ref_b, **tol), c
        assert R.close(par.pw.double().sum(0), par.ref_w, **tol) and R.close(par.pb.double().sum(0), par.ref_b, **tol), c


@pytest.mark.parametrize("which", ["flush", "classes", "limit"])
def test_twin_weight_gradient_batch(which):
    be = _be()
    cases = R.batch_cases(which)
    fins = True if which == "limit" else [i % 3 != 2 for i in range(len(cases))]
    for c, o in zip(cases, R.run_backward_weight_batch(be, cases, fins)):
        tol = R.tol_wgrad(c.rows)
        if o.gw is not None:
            assert R.close(o.gw, o.ref_w, **tol) and R.close(o.gb, o.ref_b, **tol), c
        else:
            assert R.close(o.pw.double().sum(0), o.ref_w, **tol) and R.close(o.pb.double().sum(0), o.ref_b, **tol), c


def test_twin_weight_gradient_batch_rejects_33_products():
    assert R.run_backward_weight_batch(_be(), R.batch_cases("over"), True, expect_rc_zero=False) != 0
