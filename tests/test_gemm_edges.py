"""The dense-layer GEMMs (csrc/qa_gemm.hip) through the C ABI against float64 at their tile, tail, split and alignment edges, under every
forced tile configuration of both kernel templates.  Operands are windows of NaN-poisoned allocations, outputs windows of sentinel-filled
ones, scratch is sentinel-filled with a guard tail (tests/gemm_ref.py); every shape is small.  Tolerances are the project's own
(test_gemm_layers._tol for forward / input gradient, test_hip_backward_matches_fp32_torch's for weight / bias gradients); nothing is
excluded.  Each test asserts through the restated plans (checked here against the library's own *_layout / *_scratch_bytes, which launch
nothing) that its cases hit the kernel, tile, k-tile count, workgroup total, split and vector widths they are there for."""
import ctypes as C
from dataclasses import replace

import pytest

from tests import gemm_ref as R

pytestmark = pytest.mark.gpu

FEATURES = R.WGRAD_FEATURES


@pytest.fixture
def be():
    from quadrupedal_agility_amd import _capi
    lib = _capi.load_library()
    try:
        yield R.Backend(lib, "qa_", "cuda")
    finally:
        lib.qa_gemm_force_config(-1)


def _force(be, cfg):
    be.lib.qa_gemm_force_config(cfg)


def _layout(be, name, rows, k, n):
    lay = (C.c_int64 * 5)()
    assert be.fn(name)(rows, k, n, lay) == 0
    return [int(v) for v in lay]


@pytest.mark.parametrize("forced", (-1,) + R.CFGS + (4, 7, 15, 99))
def test_restated_plans_equal_the_library_layouts(be, forced):
    _force(be, forced)
    shapes = [(rows, k, n) for rows in R.WGRAD_ROWS + (40, 3072) for k, n in FEATURES + ((671, 512), (256, 128), (130, 3))]
    for rows, k, n in shapes:
        assert _layout(be, "linear_backward_weight_layout", rows, k, n) == R.wgrad_layout(rows, k, n, forced), (rows, k, n)
        assert be.fn("linear_backward_weight_scratch_bytes")(rows, k, n) == R.wgrad_scratch_bytes(rows, k, n, forced), (rows, k, n)
        assert _layout(be, "linear_backward_weight_batch_layout", rows, k, n) == R.wgrad_batch_layout(rows, k, n), (rows, k, n)
        assert be.fn("linear_backward_weight_batch_scratch_bytes")(rows, k, n) == R.wgrad_batch_scratch_bytes(rows, k, n), (rows, k, n)
    for rows, k, n in R.SPLIT_SHAPES + ((256, 62400, 128), (37, 5000, 8)):
        assert be.fn("linear_forward_split_scratch_bytes")(rows, k, n) == R.fwd_split_scratch_bytes(rows, k, n), (rows, k, n)


def _check_layer(be, product, c, want, cfg):
    out = (R.run_forward if product == "forward" else R.run_backward_input)(be, c)
    if want:
        assert out.vec == want, (c, out.vec, want)
    kred = c.k if product == "forward" else c.n
    assert R.close(out.got, out.ref, **R.tol_layer(kred)), (product, cfg, c, R.worst(out.got, out.ref))
    return R.layer_launch(product, c, out.vec, cfg)


@pytest.mark.parametrize("group", ["counts", "klens", "vecs", "ring", "dma_counts", "totals", "placement"])
@pytest.mark.parametrize("cfg", R.CFGS)
@pytest.mark.parametrize("product", ["forward", "backward_input"])
def test_layer_edges_under_every_tile(be, product, cfg, group):
    _force(be, cfg)
    cases = R.layer_cases(product, cfg)[group]
    launches = [_check_layer(be, product, c, want, cfg) for c, want in cases]
    vecs = {want[:2] for _, want in cases if want}
    if group == "vecs":
        assert vecs == {(4, 4), (4, 1), (1, 4), (1, 1)} and [l.dma for l in launches] == [cfg >= 10, False, False, False]
    if group == "klens":
        assert {l.k_tiles for l in launches} == {1, 2, 3, 4}
    if group == "ring":
        want = [(cfg >= 10, 1), (cfg >= 10, 2), (cfg >= 10, 3), (cfg >= 10, 4), (False, 2)]          # the ring at 1..4 tiles, and one fallback
        assert [(l.dma, l.k_tiles) for l in launches] == want
    if group == "dma_counts":
        assert all(l.dma == (cfg >= 10) for l in launches)
        ba, bb = R.tile_dims(cfg)
        step = 1 if product == "forward" else 4
        assert {bb - 1, bb, bb + 1} <= {c.rows for c, _ in cases} and {ba - step, ba, ba + step} <= {(c.n if product == "forward" else c.k) for c, _ in cases}
        assert {c.oc for c, _ in cases} == {"a", "b", "c"} and {want[2] for _, want in cases} == {1, 4}
    if group == "placement":
        # what the LDS-DMA kernel can take of them: 16-byte operands and at least 4 outputs per row (an input gradient 70 wide reads its weight 4 bytes at a time)
        takes = [c.wc == "a" and (c.n if product == "forward" else c.k) >= 4 and (product == "forward" or c.k % 4 == 0) for c, _ in cases]
        assert [l.dma for l in launches] == [cfg >= 10 and t for t in takes] and sum(takes) >= 5
        assert {want[2] for (_, want), t in zip(cases, takes) if t} == {1, 4}
    if group == "totals":
        assert sorted(l.workgroups for l in launches) == [1, 7, 8, 9, 15] and all(l.dma == (cfg >= 10) and (l.ba, l.bb) == R.tile_dims(cfg) for l in launches)


@pytest.mark.parametrize("cfg", [2, 13])
@pytest.mark.parametrize("product", ["forward", "backward_input"])
def test_every_activation_and_its_derivative(be, product, cfg):
    _force(be, cfg)
    cases = R.activation_cases(product)
    assert [c.act for c, _ in cases] == list(R.ACTS)
    for c, want in cases:
        assert _check_layer(be, product, c, want, cfg).dma == (cfg == 13)


@pytest.mark.parametrize("cfg", (-1,) + R.CFGS)
def test_split_forward_edges(be, cfg):
    _force(be, cfg)
    ran_dma = []
    for c in R.split_cases():
        one, two = R.run_forward_split(be, c)
        assert R.same_bits(one.got, two.got), c
        assert R.close(one.got, one.ref, **R.tol_layer(c.k)), (cfg, c, R.worst(one.got, one.ref))
        ran_dma.append(R.split_launch(c, one.vec, cfg).dma)
    assert ran_dma == [False] * len(R.SPLIT_SHAPES) + [cfg >= 10]           # the issue's five shapes fall back; the sixth is the LDS-DMA kernel with split partials


def _check_wgrad(c, fin, par):
    """a finished call and a parts-only call of the same product"""
    tol = R.tol_wgrad(c.rows)
    assert fin.lay == par.lay
    assert R.same_bits(fin.pw, par.pw) and R.same_bits(fin.pb, par.pb), c                                   # two runs, bit for bit
    assert R.close(par.pw.double().sum(0), par.ref_w, **tol), (c, R.worst(par.pw.double().sum(0), par.ref_w))
    assert R.close(par.pb.double().sum(0), par.ref_b, **tol), (c, R.worst(par.pb.double().sum(0), par.ref_b))
    assert R.same_bits(fin.gw, R.ordered_sum_f32(list(fin.pw))), c                                           # the documented fixed order, no tolerance
    assert R.same_bits(fin.gb, R.ordered_sum_f32(list(fin.pb))), c
    assert R.close(fin.gw, fin.ref_w, **tol) and R.close(fin.gb, fin.ref_b, **tol), c


@pytest.mark.parametrize("k,n", FEATURES)
@pytest.mark.parametrize("cfg", R.CFGS)
def test_weight_gradient_edges_under_every_tile(be, cfg, k, n):
    _force(be, cfg)
    splits, idle_rows, vecs, dma = set(), 0, set(), set()
    for c, want in R.wgrad_cases(k, n):
        fin, par = R.run_backward_weight(be, c, True), R.run_backward_weight(be, c, False)
        assert fin.vec[:2] == want == par.vec[:2], (c, fin.vec, want)
        assert fin.lay == R.wgrad_layout(c.rows, k, n, cfg), c
        _check_wgrad(c, fin, par)
        L = R.wgrad_launch(c, fin.vec, cfg)
        _, s, kps = R.wgrad_plan(c.rows, k, n, cfg)
        assert fin.lay[0] == s == L.nsplit and fin.lay[2] == s * L.na
        # k-tile t of a split rides on a-tile t % na: an a-tile beyond the split's k-tiles carries none, and its bias row is written zeros
        for z in range(s):
            tiles = -(-(min(c.rows, (z + 1) * kps) - z * kps) // 16)
            for at in range(tiles, L.na):
                assert bool((fin.pb[z * L.na + at] == 0).all()), (c, z, at)
                idle_rows += 1
        if (k, n) == (300, 7) and c.rows <= 16 and L.ba == 64:
            assert L.na == 5 and int((fin.pb == 0).all(1).sum()) == 4, c
        splits.add(s); vecs.add(fin.vec[:2]); dma.add(L.dma)
    assert splits == {1, 2, 3}
    assert (idle_rows > 0) == (-(-k // R.tile_dims(cfg)[0]) > 1)
    if k % 4 == 0 and n % 4 == 0:
        assert vecs == {(4, 4), (4, 1), (1, 4), (1, 1)} and dma == ({True, False} if cfg >= 10 else {False})


def _check_batch(be, cases, fins):
    outs = R.run_backward_weight_batch(be, cases, fins)
    for c, o in zip(cases, outs):
        assert o.lay == R.wgrad_batch_layout(c.rows, c.k, c.n), c
        tol = R.tol_wgrad(c.rows)
        assert R.close(o.pw.double().sum(0), o.ref_w, **tol) and R.close(o.pb.double().sum(0), o.ref_b, **tol), c
        if o.gw is not None:
            assert R.close(o.gw, o.ref_w, **tol) and R.close(o.gb, o.ref_b, **tol), c
    return outs


def test_grouped_weight_gradient_flushes_a_full_group(be):
    """14 products of one vector class: the group holds 12, so a launch of 12 and a second one of 2"""
    cases = R.batch_cases("flush")
    outs = _check_batch(be, cases, [i % 3 != 2 for i in range(len(cases))])
    assert len(outs) == 14 and {o.vec[:2] for o in outs} == {(4, 4)} and {o.lay[0] for o in outs} == {1, 2, 3}
    again = R.run_backward_weight_batch(be, cases, False)
    assert all(R.same_bits(a.pw, o.pw) and R.same_bits(a.pb, o.pb) for a, o in zip(again, outs))


def test_grouped_weight_gradient_in_all_four_vector_classes(be):
    cases = R.batch_cases("classes")
    outs = _check_batch(be, cases, [i % 2 == 0 for i in range(len(cases))])
    assert {o.vec[:2] for o in outs} == {(4, 4), (4, 1), (1, 4), (1, 1)}
    assert outs[1].vec[:2] == (4, 1) and cases[1].k % 4 != 0 and outs[5].vec[:2] == (4, 4) and cases[5].k % 4 != 0      # the x-pad path: NaN padding read, reaching no output


def test_grouped_weight_gradient_takes_32_finished_products_and_rejects_33(be):
    outs = _check_batch(be, R.batch_cases("limit"), True)
    assert len(outs) == 32 and all(o.gw is not None for o in outs)              # 64 reductions: the limit
    assert R.run_backward_weight_batch(be, R.batch_cases("over"), True, expect_rc_zero=False) != 0
    assert b"qa_linear_backward_weight_batch" in be.lib.qa_last_error()


def test_forced_window_tile_runs_the_linear_products_as_64_x_64(be):
    """a forced 4 (32 x 128, a window-GEMM tile) used to plan the bias slabs for 32-wide a-tiles and launch 64-wide ones: for in_features > 32 the
    reduction then added bias rows that no workgroup had written"""
    c = R.Layer(rows=40, k=100, n=12, oc="d", seed=40)
    _force(be, 4)
    fin, par = R.run_backward_weight(be, c, True), R.run_backward_weight(be, c, False)
    assert fin.lay == R.wgrad_layout(40, 100, 12, 2) and fin.lay[2] == 2
    _check_wgrad(c, fin, par)
    _force(be, 2)
    as2 = R.run_backward_weight(be, c, True)
    assert R.same_bits(as2.gw, fin.gw) and R.same_bits(as2.gb, fin.gb)
    for f in (5, 9):
        _force(be, f)
        got = R.run_forward(be, c).got
        _force(be, 2)
        assert R.same_bits(got, R.run_forward(be, c).got)


@pytest.mark.parametrize("forced", [15, 99])
def test_forced_value_outside_every_table_is_no_force(be, forced):
    """planning used to take 128-wide a-tiles for it and the launch (not DMA-eligible) 64-wide ones: more bias rows written than scratch holds"""
    for c in (R.Layer(rows=40, k=100, n=12, oc="d", seed=41), R.Layer(rows=40, k=132, n=12, xc="b", gc="c", oc="e", seed=42), R.Layer(rows=48, k=300, n=7, seed=43)):
        _force(be, -1)
        plain = (R.run_forward(be, c), R.run_backward_input(be, c), R.run_backward_weight(be, c, True), R.run_forward_split(be, replace(c, k=520, n=8, oc="a"))[0])
        _force(be, forced)
        same = (R.run_forward(be, c), R.run_backward_input(be, c), R.run_backward_weight(be, c, True), R.run_forward_split(be, replace(c, k=520, n=8, oc="a"))[0])
        assert same[2].lay == plain[2].lay == R.wgrad_layout(c.rows, c.k, c.n, -1)
        assert R.same_bits(plain[0].got, same[0].got) and R.same_bits(plain[1].got, same[1].got) and R.same_bits(plain[3].got, same[3].got), c
        assert R.same_bits(plain[2].gw, same[2].gw) and R.same_bits(plain[2].gb, same[2].gb), c
        _check_wgrad(c, same[2], R.run_backward_weight(be, c, False))
