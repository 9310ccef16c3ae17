"""The learner's loss and reduction kernels (csrc/qa_learner.hip, the fused GAE of csrc/qa_sim.hip) through the C ABI against float64 at their
structural edges: block and lane boundaries, template switches, the branches of the parts reductions, ragged tails, exact ties.  Operands are windows
of NaN-poisoned allocations, outputs windows of sentinel-filled ones, scratch is exactly what *_scratch_bytes() declares with a guard tail behind it
(tests/learner_ref.py); every shape is the smallest that reaches its edge.  Nothing is excluded from a comparison.  Each test asserts through the
restated plans (checked here against the library's own *_scratch_bytes, which launch nothing) that its cases hit the template, block count, tail
and branch they are there for.

Tolerances are the project's own, by name (learner_ref.GAE_TOL_*, tol_elu_bias, tol_narrow, NORM_TOL_*, tol_reduce, pair_loss_close / PAIR_TOL_GRAD),
except for the outputs of the fp32 kernels that had none.  For those the worst error of a numpy float32 evaluation of the same reference formula against
the float64 reference was measured on the CPU over the same cases (learner_ref.measure_gae_offset / measure_adam; tests/test_learner_edges_cpu.py
re-measures and holds the constants in learner_ref to 4 x the measurement):

    output                                         fp32 evaluation, worst |error|     tolerance (4 x)      constant in learner_ref
    GAE, rewards +100: returns                     6.73e-4                            2.69e-3              TOL_GAE_OFFSET_RET
    GAE, rewards +100: normalised advantages       7.22e-6                            2.89e-5              TOL_GAE_OFFSET_ADV
    one Adam step: parameter                       1.191e-7                           4.77e-7              TOL_ADAM["p"]
    one Adam step: exp_avg                         2.96e-8                            1.185e-7             TOL_ADAM["m"]
    one Adam step: exp_avg_sq                      3.09e-9                            1.236e-8             TOL_ADAM["v"]
    two Adam steps in a row: parameter             2.313e-7                           9.25e-7              TOL_ADAM_TWICE["p"]
    two Adam steps in a row: exp_avg               7.40e-8                            2.96e-7              TOL_ADAM_TWICE["m"]
    two Adam steps in a row: exp_avg_sq            6.37e-9                            2.549e-8             TOL_ADAM_TWICE["v"]

The normaliser keeps and computes its moments in double, so its data set with means ~1e3 and spreads ~1e-2 is held to the project's own double-precision
bounds (NORM_TOL_MEAN / NORM_TOL_VAR), not to an fp32 measurement.
"""
import numpy as np
import pytest
import torch

from tests import learner_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture
def be():
    from quadrupedal_agility_amd import _capi
    return R.Backend(_capi.load_library(), "qa_", "cuda")


# ---------------------------------------------------------------- the restated plans against the entry points that launch nothing
def test_restated_plans_equal_the_library_scratch_sizes(be):
    for rows in R.ELU_ROWCOUNTS + tuple(64 * n for n in R.ELU_FINISH_BLOCKS):
        for cols in R.ELU_COLS:
            assert be.fn("elu_backward_bias_scratch_bytes")(rows, cols) == 4 * cols * R.elu_plan(rows, cols).nblocks, (rows, cols)
    for rows in R.NARROW_ROWS + (2048, 2304, 2305, 32512, 40000):
        for o, k in ((1, 1), (5, 257), (32, 128)):
            assert be.fn("narrow_wgrad_scratch_bytes")(rows, o, k) == R.narrow_scratch_bytes(rows, o, k), (rows, o, k)
    for rows in R.PAIR_ROWS + (65537,):
        assert be.fn("pair_loss_scratch_bytes")(rows) == 4 * R.pair_blocks(rows)
    # the slab clamp at both ends: 8 rows per slab up to 2,048 rows, 128 from 32,513 on; 32,768 | 32,769 is the 256 | 257 slab edge
    assert [R.narrow_plan(r)[:2] for r in (1, 7, 8, 9, 2048, 2049, 32768, 32769)] == [(8, 1), (8, 1), (8, 1), (8, 2), (8, 256), (9, 228), (128, 256), (128, 257)]


# ---------------------------------------------------------------- GAE
def test_gae_edges(be):
    plans = {}
    for c in R.gae_cases():
        o = R.run_gae(be, c)
        assert R.close(o.ret, o.ref_ret, **R.GAE_TOL_RET), (c, R.worst(o.ret, o.ref_ret))
        assert R.close(o.adv, o.ref_adv, **R.GAE_TOL_ADV), (c, R.worst(o.adv, o.ref_adv))
        plans.setdefault(R.gae_plan(c.N), set()).add((c.normalize, c.dones))
    # one block, two, the cap of 128 blocks exactly filled (no stride), the cap with a second round of one env and of 7,232
    assert set(plans) == {(1, False), (2, False), (128, False), (128, True)}
    assert {c.N for c in R.gae_cases() if R.gae_plan(c.N) == (128, True)} == {32769, 40000} and R.gae_plan(32768) == (128, False)
    assert {n for v in plans.values() for n, _ in v} == {True, False} and {d for v in plans.values() for _, d in v} == set(R.GAE_DONES)
    assert all({n for n, _ in plans[p]} == {True, False} for p in ((128, False), (128, True)))
    assert not any(c.normalize and c.T * c.N == 1 for c in R.gae_cases())
    # the normalising launch's own cap of 1,024 blocks: every listed shape stays under it, one more case is past it (its stride loop, over a strided scan)
    norm_plans = {R.gae_norm_plan(c.T, c.N) for c in R.gae_cases() if c.normalize}
    assert (1024, True) in norm_plans and (313, False) in norm_plans and {s for _, s in norm_plans} == {False, True}


def test_gae_with_a_common_offset(be):
    for c in R.gae_offset_cases():
        o = R.run_gae(be, c)
        assert float(o.ref_ret.abs().min()) > 90.0                      # the offset is there
        assert R.close(o.ret, o.ref_ret, atol=R.TOL_GAE_OFFSET_RET), (c, R.worst(o.ret, o.ref_ret))
        assert R.close(o.adv, o.ref_adv, atol=R.TOL_GAE_OFFSET_ADV), (c, R.worst(o.adv, o.ref_adv))
    assert {R.gae_plan(c.N)[1] for c in R.gae_offset_cases()} == {False, True}


# ---------------------------------------------------------------- ELU backward + bias
def _check_elu(be, c):
    fin, par = R.run_elu(be, c, True), R.run_elu(be, c, False)
    p = R.elu_plan(c.rows, c.cols)
    assert fin.parts.shape == (p.nblocks, c.cols)
    assert bool(((fin.gin.double() - fin.ref_gin).abs() <= R.elu_gin_bound(fin.gy, fin.f)).all()), c
    zeros = fin.y == 0
    assert bool(zeros.any()) and torch.equal(fin.gin[zeros], (fin.gy * c.alpha)[zeros]), c           # y == 0: the factor is alpha exactly (0 for ReLU)
    assert R.same_bits(fin.gin, par.gin) and R.same_bits(fin.parts, par.parts), c                      # two runs, bit for bit
    assert R.close(par.parts, par.ref_parts, **R.tol_elu_bias(min(c.rows, R.ELU_ROWS))), (c, R.worst(par.parts, par.ref_parts))
    assert R.same_bits(fin.gb.reshape(-1), R.colsum_order_f32(list(fin.parts))), c                     # the documented fixed order, no tolerance
    assert R.close(fin.gb.reshape(-1), fin.ref_gb, **R.tol_elu_bias(c.rows)), (c, R.worst(fin.gb.reshape(-1), fin.ref_gb))
    return p, bool((fin.y < 0).any())


def test_elu_backward_bias_edges(be):
    seen = {}
    for c in R.elu_cases():
        p, neg = _check_elu(be, c)
        seen.setdefault(c.cols, []).append((c, p, neg))
    # both sides of every CW switch, and the 256-wide template with a ragged second / third column pass
    assert {cols: v[0][1].cw for cols, v in seen.items()} == {1: 32, 32: 32, 33: 64, 64: 64, 65: 128, 128: 128, 129: 256, 256: 256, 257: 256, 513: 256}
    assert seen[257][0][1][3:5] == (2, True) and seen[513][0][1][3:5] == (3, True) and seen[256][0][1][3:5] == (1, False)
    for cols, v in seen.items():
        assert {c.rows for c, _, _ in v} >= set(R.ELU_ROWCOUNTS) and {c.alpha for c, _, _ in v} == {0.0, 1.0}, cols
        assert {p.nblocks for _, p, _ in v} == {1, 2, 3} and {p.last_rows for _, p, _ in v} >= {1, 7, 8, 9, 63, 64}, cols
        assert {(p.unrolled, p.tail) for _, p, _ in v} >= {(False, True), (True, True)}, cols          # rows too few for the 4-row unroll; unroll and single rows
        assert any(neg for c, _, neg in v if c.alpha == 1.0) and not any(neg for c, _, neg in v if c.alpha == 0.0), cols
    # the unroll boundary `r + 3 RL < r1` of each template: RL = 8, 4, 2, 1 -> a lane's first unrolled round needs more than 24, 12, 6, 3 rows
    assert [R.elu_plan(r, 32).unrolled for r in (9, 63)] == [False, True] and [R.elu_plan(r, 257).unrolled for r in (1, 7)] == [False, True]
    assert R.elu_plan(64, 257).tail is False and R.elu_plan(65, 257).tail is True


def test_elu_backward_bias_finish_unroll_edges(be):
    plans = [(_check_elu(be, c)[0], c) for c in R.elu_finish_cases()]
    assert [p.nblocks for p, _ in plans] == list(R.ELU_FINISH_BLOCKS) and all(p.cw == 64 for p, _ in plans)
    # `b + 24 < nblocks`: fewer parts than lanes, one per lane, 24 | 25 the first unrolled round, 32 | 33 its last lane, 57 a second round
    assert [(p.finish_unrolled, p.finish_rounds) for p, _ in plans] == [(False, 0), (False, 0), (False, 0), (False, 0), (True, 1), (True, 1), (True, 1), (True, 2)]
    assert {c.alpha for _, c in plans} == {0.0, 1.0}


# ---------------------------------------------------------------- narrow weight gradient
def test_narrow_wgrad_edges(be):
    seen = []
    for c in R.narrow_cases():
        a, b = R.run_narrow(be, c), R.run_narrow(be, c)
        assert a.nbytes == R.narrow_scratch_bytes(c.rows, c.o, c.k), c
        assert R.same_bits(a.gw, b.gw) and R.same_bits(a.gb, b.gb), c                                  # fixed order: bit-reproducible
        assert R.close(a.gw, a.ref_w, **R.tol_narrow(c.rows)), (c, R.worst(a.gw, a.ref_w))
        assert R.close(a.gb, a.ref_b, **R.tol_narrow(c.rows)), (c, R.worst(a.gb, a.ref_b))
        seen.append((c, R.narrow_omax(c.o)) + R.narrow_plan(c.rows))
    assert {(c.o, om) for c, om, *_ in seen} == {(1, 1), (2, 4), (4, 4), (5, 16), (16, 16), (17, 32), (32, 32)}      # both sides of every OMAX switch
    for o in R.NARROW_O:
        assert {c.k for c, *_ in seen if c.o == o} >= set(R.NARROW_K), o                                # K = 255 | 256 | 257 and two column rounds plus one
    assert {c.rows for c, *_ in seen} == set(R.NARROW_ROWS)
    assert all(c.k <= 128 for c, *_ in seen if c.rows > 2049)
    # the lower clamp with one short slab (< 4 rows: no unrolled round), exactly one slab, a second slab of one row; just past it; the upper clamp at 256 | 257 slabs
    assert {(sr, nb, last) for c, _, sr, nb, last in seen} >= {(8, 1, 1), (8, 1, 3), (8, 1, 7), (8, 1, 8), (8, 2, 1), (8, 2, 5), (9, 228, 6), (128, 256, 128), (128, 257, 1)}
    assert {R.narrow_omax(c.o) for c, _, sr, nb, _ in seen if (sr, nb) == (128, 257)} >= {4, 32}
    assert R.run_narrow(be, R.Narrow(9, 33, 7), expect_rc_zero=False) != 0 and b"qa_narrow_wgrad" in be.lib.qa_last_error()


# ---------------------------------------------------------------- running-moment normaliser
def test_normalizer_update_edges(be):
    blocks, ks, lens = set(), set(), set()
    for c in R.norm_cases():
        got, ref = R.run_normalizer(be, c)
        for call, ((m, v, n), (rm, rv, rn)) in enumerate(zip(got, ref)):
            assert R.close(m, rm, **R.NORM_TOL_MEAN), (c, call, R.worst(m, rm))
            assert R.close(v, rv, **R.NORM_TOL_VAR), (c, call, R.worst(v, rv))
            assert n == rn == 37.0 + (call + 1) * sum(c.lengths), c
        blocks.add(-(-c.d // R.NORM_COLS)); ks.add(len(c.lengths)); lens |= set(c.lengths)
    assert {c.d for c in R.norm_cases()} == set(R.NORM_D) and blocks == {1, 2, 7, 8} and ks == {1, 2, 3, 4} and lens == set(R.NORM_LENGTHS)
    assert all({len(c.lengths) for c in R.norm_cases() if c.d == d} == {1, 2, 3, 4} for d in R.NORM_D)
    assert any(len(set(c.lengths)) > 1 for c in R.norm_cases())                                        # lengths mixed within one call
    # row lanes (unrolled, single-row, idle): one row, a lane short, every lane once, one lane twice; the 8 x 64 unroll for 63 lanes, for all with no row left, and one left
    assert [R.norm_plan(n) for n in (1, 63, 64, 65, 511, 512, 513)] == [(0, 1, 63), (0, 63, 1), (0, 64, 0), (0, 64, 0), (63, 1, 0), (64, 0, 0), (64, 1, 0)]
    assert any(c.lengths == (1,) for c in R.norm_cases())                                              # a batch of one row: zero variance, merged


def test_normalizer_update_on_offset_data(be):
    c = R.norm_offset_case()
    got, ref = R.run_normalizer(be, c)
    assert float(ref[1][0].min()) > 900.0 and float(ref[1][1].max()) < 1.0
    for (m, v, n), (rm, rv, rn) in zip(got, ref):
        assert R.close(m, rm, **R.NORM_TOL_MEAN) and R.close(v, rv, **R.NORM_TOL_VAR) and n == rn, (R.worst(m, rm), R.worst(v, rv))
    assert float((ref[1][0] ** 2 / ref[1][1]).min()) > 1e9          # mean^2 / var: what a single-pass variance in fp32, or fp32 batch sums, cannot resolve


def test_normalizer_refusals_and_apply(be):
    assert all(rc != 0 for rc in R.normalizer_refusals(be))
    for rows, d in ((37, 15), (1, 1), (3, 128)):
        y, ref = R.run_normalizer_apply(be, rows, d)
        assert R.close(y, ref, **R.NORM_TOL_APPLY), (rows, d, R.worst(y, ref))
        if rows * d > 100:
            assert (rows * d) % 256 != 0 and bool((ref == R.f32(1.5)).any()) and bool((ref == -R.f32(1.5)).any())      # both clips active


# ---------------------------------------------------------------- gradients in parts
def test_grad_reduce_edges(be):
    shapes = R.reduce_cases()
    one, two = R.run_grad_reduce(be, shapes), R.run_grad_reduce(be, shapes)
    for (n, p), (got, src), (again, _) in zip(shapes, one, two):
        assert R.same_bits(got, again), (n, p)
        assert R.same_bits(got, R.parts_order_sum(src)), (n, p, R.parts_branch(p))                     # the promised order, no tolerance
        assert R.close(got, src.double().sum(0), **R.tol_reduce(p)), (n, p, R.worst(got, src.double().sum(0)))
    assert {(p, R.parts_branch(p)) for _, p in shapes} >= {(16, "narrow"), (17, "wide")} and {n for n, _ in shapes} == set(R.REDUCE_NUMEL)
    assert all({n for n, p in shapes if p == q} == set(R.REDUCE_NUMEL) for q in R.PARTS_NARROW + R.PARTS_WIDE)


def _stepped_adam(sizes):
    """a torch Adam over zero tensors of these sizes with its state created, and its ClipAdam"""
    from quadrupedal_agility_amd.rsl_rl.algorithms import fused
    ps = [torch.nn.Parameter(torch.zeros(n, device="cuda")) for n in sizes]
    opt = torch.optim.Adam(ps, lr=torch.tensor(1e-3, device="cuda"), fused=True, capturable=True)
    for p in ps:
        p.grad = torch.zeros_like(p)
    opt.step()
    return ps, fused.ClipAdam(opt, 1.0)


def _check_chunk_table(tab, sizes, chunk, first_tensor=0, first_chunk=0):
    """tensors [first_tensor, +len(sizes)) of a chunk table: every tensor covered once, in order; one that may be handed more than WIDE_PARTS parts (numel <= CHUNK,
    the `can` of ClipAdam._prepare) in chunks of at most 32 elements"""
    ct, cs, cl = (tab[k].cpu().tolist()[first_chunk:] for k in ("chunk_tensor", "chunk_start", "chunk_len"))
    for i, n in enumerate(sizes):
        mine = [(s, l) for c, s, l in zip(ct, cs, cl) if c == first_tensor + i]
        assert sum(l for _, l in mine) == n and [s for s, _ in mine] == [sum(l for _, l in mine[:j]) for j in range(len(mine))], (n, mine[:3])
        assert (max(l for _, l in mine) <= 32) == (n <= chunk), (n, mine[:3])
    return len([c for c in ct if first_tensor <= c < first_tensor + len(sizes)])


def test_chunk_tables_keep_many_part_tensors_in_32_element_chunks():
    """what the many-parts branch of adam_reduce_chunk rests on -- it adds the first 32 elements of a chunk and no more -- for the tables of ClipAdam and the
    merged ones of ClipAdamPair: a tensor of at most CHUNK elements has chunks of at most 32, and a larger one is never handed over with more than WIDE_PARTS
    parts (ClipAdam finishes them first; the pair declines the step and leaves them to the two single steps)"""
    from quadrupedal_agility_amd.rsl_rl.algorithms import fused
    sizes_a, sizes_b = (1, 31, 32, 33, 512, 2047, 2048, 2049, 5000), (2048, 7, 4097, 64)
    (pa, ca), (pb, cb) = _stepped_adam(sizes_a), _stepped_adam(sizes_b)
    assert (ca.WIDE_PARTS, ca.SMALL_CHUNK, ca.CHUNK) == (R.QA_REDUCE_WIDE, 32, R.ADAM_CHUNK)
    na = _check_chunk_table(ca._prepare()["tab"], sizes_a, ca.CHUNK)
    pair = fused.ClipAdamPair(ca, cb)
    assert pair.warm() is True, pair.why_not                          # builds the merged tables, launches nothing
    m = pair._tab
    assert m["n"] == len(sizes_a) + len(sizes_b) and _check_chunk_table(m, sizes_a, ca.CHUNK) == na == m["ta"]["num_chunks"]
    assert _check_chunk_table(m, sizes_b, cb.CHUNK, first_tensor=len(sizes_a), first_chunk=na) == m["tb"]["num_chunks"] == m["num_chunks"] - na
    # parts registered the way the backward functions register them
    for p, handed_over in ((pa[-1], False), (pa[-3], True)):
        fused.register_grad_parts(p, torch.zeros(17, p.numel(), device="cuda"), 17, p.numel(), p.grad)
        try:
            dry = pair.step(dry=True)                                   # the pair never finishes parts itself
            assert dry is handed_over and fused.pending_grads() == 1 and (pair.why_not is None) == handed_over, (p.numel(), pair.why_not)
            pre = ca._prepare()                                         # the single step finishes what it cannot take, and only that
            assert (pre["pend"] is not None) == handed_over and fused.pending_grads() == (1 if handed_over else 0), p.numel()
        finally:
            fused.flush_pending_grads([p])
        assert fused.pending_grads() == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------- clip + Adam
def _check_adam(outs, tol=R.TOL_ADAM):
    for o in outs:
        for i, (got, ref) in enumerate(zip(o.tensors, o.ref)):
            for k in "pmv":
                assert R.close(got[k], ref[k], atol=tol[k]), (i, k, R.worst(got[k], ref[k]))


def _check_head(o, c):
    h, r = [float(x) for x in o.head], o.ref_head
    assert h[0] == pytest.approx(r["coef"], rel=1e-6) and h[1] == pytest.approx(r["bc1"], rel=1e-5) and h[2] == pytest.approx(r["bc2s"], rel=1e-5)
    assert h[3] == pytest.approx(r["norm"], rel=1e-6) and (r["norm"] > 0) == (c.max_norm > 0)
    assert o.steps == [c.step0 + 1.0] * len(c.sizes)


@pytest.mark.parametrize("entry", ["step", "hostgrads"])
def test_clip_adam_step_edges(be, entry):
    cs = R.adam_measure_cases()[:4]
    assert all(c.sizes == (1, 255, 256, 257, 2047, 2048, 2049) for c in cs) and R.adam_chunks(cs[0])[2] == [1, 255, 256, 257, 2047, 2048, 2048, 1]
    coefs = []
    for c in cs:
        for spare in ((0,) if c.max_norm > 0 else (0, 1)):           # without clipping: finalize + update, and with the spare float the single launch
            o, = R.run_adam(be, entry, c, spare=spare)
            _check_adam([o]); _check_head(o, c)
            assert o.ticket == (0 if spare else None)
            coefs.append(o.ref_head["coef"])
    assert min(coefs) < 0.1 and 1.0 in coefs                         # a clipped and an unclipped step
    assert {(c.max_norm > 0, c.wd > 0, c.step0) for c in cs} == {(True, False, 0), (True, True, 1000), (False, True, 0), (False, False, 1000)}
    # the single launch twice in a row: the ticket word is back at 0 both times and the counters advanced twice
    assert R.adam_twice_cases() == cs[2:]
    for c in R.adam_twice_cases():
        o, = R.run_adam(be, entry, c, spare=1, calls=2)
        _check_adam([o], R.TOL_ADAM_TWICE)
        assert o.ticket == 0 and o.steps == [c.step0 + 2.0] * len(c.sizes)


def test_clip_adam_step_reduce_edges(be):
    cs = R.adam_measure_cases()[4:]
    branches = set()
    for c in cs:
        o, = R.run_adam(be, "reduce", c)
        again, = R.run_adam(be, "reduce", c)
        _check_adam([o]); _check_head(o, c)
        T = R.adam_draw(c)
        for t, (got, ag, ref, d) in enumerate(zip(o.tensors, again.tensors, o.ref, T)):
            k, chunk = c.parts_of(t), c.chunk_of(t)
            if k:
                branches.add((k, R.parts_branch(k)))
                assert k <= R.QA_REDUCE_WIDE or chunk <= 32, c                                         # what the header asks of the caller's table
                assert d["src"].shape == (k, c.sizes[t]) and R.same_bits(got["g"], R.parts_order_sum(d["src"])), (c, t, k)      # written where .grad is, in the promised order
                assert R.close(got["g"], ref["g"], **R.tol_reduce(k)), (c, t)
            assert all(R.same_bits(got[x], ag[x]) for x in "pmvg"), (c, t)
    assert {k for k, _ in branches} == set(R.PARTS_NARROW + R.PARTS_WIDE) and {(16, "narrow"), (17, "wide")} <= branches
    assert any(c.parts_of(t) in R.PARTS_NARROW and n == 2049 for c in cs for t, n in enumerate(c.sizes))
    assert all(n <= 70 for c in cs for t, n in enumerate(c.sizes) if c.parts_of(t) > 16)


def test_clip_adam_pair_step_edges(be):
    cs = R.adam_measure_cases()
    a, b = cs[6], cs[7]
    na, nb = len(R.adam_chunks(a)[0]), len(R.adam_chunks(b)[0])
    assert na > 256 and nb > 256                                     # more than 256 chunks on each side of the split: the finalize launch's second round
    outs = R.run_adam(be, "pair", a, b)
    _check_adam(outs)
    _check_head(outs[0], a); _check_head(outs[1], b)
    assert outs[0].ref_head["coef"] == 1.0 and outs[1].ref_head["coef"] < 0.1 and outs[0].ticket != R.SENTINEL
    singles = R.run_adam(be, "reduce", a) + R.run_adam(be, "reduce", b)
    for o, s in zip(outs, singles):                                  # each half is the single optimiser's step, bit for bit
        assert all(R.same_bits(x[k], y[k]) for x, y in zip(o.tensors, s.tensors) for k in "pmvg")


# ---------------------------------------------------------------- pair losses
def test_pair_loss_edges(be):
    seen, njobs = [], set()
    for jobs in R.pair_job_lists():
        two = R.run_pair_losses(be, jobs)                            # two launches on the same scratch
        njobs.add(len(jobs))
        for c, a, b in zip(jobs, *two):
            s = R.run_pair_loss(be, c)
            assert R.pair_loss_close(s.loss, s.ref_loss) and R.close(s.grad, s.ref_grad, **R.PAIR_TOL_GRAD), (c, s.loss, s.ref_loss, R.worst(s.grad, s.ref_grad))
            assert R.pair_loss_close(a.loss, a.ref_loss) and R.close(a.grad, a.ref_grad, **R.PAIR_TOL_GRAD), (c, a.loss, a.ref_loss, R.worst(a.grad, a.ref_grad))
            assert np.float32(a.loss).tobytes() == np.float32(b.loss).tobytes() == np.float32(s.loss).tobytes() and R.same_bits(a.grad, b.grad), c
            assert R.same_bits(a.grad, s.grad * np.float32(c.scale) if c.scale else s.grad), c        # qa_pair_losses == qa_pair_loss (x the scale), bit for bit
            if c.mode == R.ROW_L2:
                assert bool((a.grad[a.zero_row] == 0).all()) and bool((s.grad[s.zero_row] == 0).all()), c
            else:
                assert bool((a.ref_grad[a.zero_row] == 0).all())
            seen.append((c.cols, c.rows, c.mode, bool(c.scale), R.pair_path(c.cols), R.pair_blocks(c.rows)))
    assert njobs == {1, 2, 3, 4}
    assert {(cols, path) for cols, _, _, _, path, _ in seen} == {(1, "lds"), (46, "lds"), (47, "lds"), (48, "wide")}
    assert {(rows, nb) for _, rows, _, _, _, nb in seen} == {(1, 1), (3, 1), (255, 1), (256, 1), (257, 2), (65537, 257)}
    for cols in R.PAIR_COLS:
        assert {r for c, r, *_ in seen if c == cols} >= set(R.PAIR_ROWS) and {m for c, _, m, *_ in seen if c == cols} == {0, 1}, cols
    for path in ("lds", "wide"):                                     # a zero-difference row with grad_scale, on both paths and in both modes
        assert {(m, sc) for _, _, m, sc, p, _ in seen if p == path} == {(0, False), (0, True), (1, False), (1, True)}, path
    assert R.run_pair_losses(be, R.pair_job_lists()[3], expect_rc_zero=False, count=5) != 0 and b"qa_pair_losses" in be.lib.qa_last_error()


# ---------------------------------------------------------------- minibatch gather
def test_gather_rows_edges(be):
    for rows in R.GATHER_ROWS:
        for widths, block in ((R.GATHER_WIDTHS, None), (R.GATHER_WIDTHS + (2, 100, 193, 300), 2), (R.GATHER_WIDTHS, 1)):
            for got, want in R.run_gather(be, rows, widths, block):
                assert torch.equal(got, want), (rows, widths, block)
    assert len(R.GATHER_WIDTHS) == 8 and len(R.GATHER_WIDTHS + (2, 100, 193, 300)) == R.GATHER_MAX
    assert [R.gather_path(w) for w in R.GATHER_WIDTHS] == ["lane", "lane", "lane", "single", "unrolled", "unrolled", "unrolled", "unrolled"]
    assert {-(-r // 4) for r in R.GATHER_ROWS} == {1, 2}             # a ragged block of waves, a full one, a second block of one row
    assert R.run_gather(be, 3, (4,) * 13, None, expect_rc_zero=False) != 0 and b"qa_gather_rows" in be.lib.qa_last_error()


# ---------------------------------------------------------------- the objectives
def _both_sides(ok, what):
    assert all(ok.values()), (what, ok)


def test_ppo_loss_edges(be):
    blocks = {}
    for c in R.ppo_cases():
        (o, d), (again, _) = R.run_ppo(be, c), R.run_ppo(be, c)
        assert o.nbytes == 4 * R.PPO_SUMS * R.ppo_blocks(c.B), c
        _both_sides(R.ppo_close(o, c.B), c)
        assert all(R.same_bits(getattr(o, k), getattr(again, k)) for k in ("stats", "dmu", "dstd", "dvalue")), c          # fixed-order reductions, no atomics
        blocks.setdefault(R.ppo_blocks(c.B), set()).add(c.clipped_value)
        if c.B == 961:
            lp = R._normal_logp(d["actions"].double(), d["mu"].double(), d["std"].double())
            counts, away = R.surrogate_census(lp, d["old_logp"], d["advantages"], R.CLIP)
            assert len(counts) == 9 and min(counts.values()) > 0 and away > 1e-4, counts
            vc, d_clip, _ = R.value_census(d["value"], d["target_values"], d["returns"], R.CLIP)
            assert min(vc.values()) > 0 and d_clip > 1e-5, vc                                       # every value-loss branch and all three exact ties
            # the ties, where the sub-gradient is a convention: v == tv and v - tv == +-clip pass 2 (v - R) / B times c_value
            for r in (9, 10, 11):
                want = 2.0 * (float(d["value"][r]) - float(d["returns"][r])) / c.B * R.PPO_COEFS["c_value"]
                assert float(o.dvalue[r]) == pytest.approx(want, rel=2e-5), (r, c)
            zero = d["advantages"] == 0
            bound = R.PPO_COEFS["c_bound"] / c.B * (2 * (d["mu"][zero].double() + 1).clamp(max=0) + 2 * (d["mu"][zero].double() - 1).clamp(min=0))
            assert bool(zero.any()) and R.close(o.dmu[zero], bound, rtol=1e-6) and bool((bound != 0).any())                # adv == 0: the bound loss alone reaches dmu
    # one ragged block, a full one, a second block of one row; the finish kernel's 15 lanes: 15 blocks, 16 (lane 0 twice), 17
    assert sorted(blocks) == [1, 2, 15, 16, 17] and R.PPO_LANES == 15 and all(v == {0, 1} for v in blocks.values())
    assert [R.ppo_blocks(B) for B in R.PPO_B] == [1, 1, 1, 2, 15, 16, 17]


def test_hybrid_ppo_loss_edges(be):
    blocks = {}
    for c in R.hyb_cases():
        (o, d), (again, _) = R.run_hyb(be, c), R.run_hyb(be, c)
        assert o.nbytes == 4 * R.HYB_SUMS * R.ppo_blocks(c.B), c
        _both_sides(R.hyb_close(o, c.B), c)
        assert all(R.same_bits(getattr(o, k), getattr(again, k)) for k in ("out", "dlogits", "dmean", "dstd", "dvalue")), c
        blocks.setdefault(R.ppo_blocks(c.B), set()).add(c.clipped_value)
        if c.B > 2:
            assert set(d["actions"][:, 0].long().tolist()) == {0, 1, 2}
            # rows 1 and 2: one probability above 1 - eps and two below eps at once; the clamp passes no gradient, so what reaches the logits is the entropy's
            # share alone -- and the reference agrees to the tolerance above.  Row 1 took the saturated class, row 2 a starved one.
            _, _, p = R.categorical_terms(d["logits"].double(), d["actions"][:, 0])
            assert float(p[1, 1]) > 1 - R.EPS32 and float(p[1, 0]) < R.EPS32 and float(p[2, 0]) > 1 - R.EPS32 and float(p[2, 2]) < R.EPS32
            assert int(d["actions"][1, 0]) == 1 and int(d["actions"][2, 0]) == 2
            assert float(o.ref[1][1:3].abs().max()) < 1e-12 * R.UPSTREAM / c.B + 1e-15 and float(o.dlogits[1:3].abs().max()) <= 1e-7 / c.B
        if c.B == 705:
            lp_d, _, _ = R.categorical_terms(d["logits"].double(), d["actions"][:, 0])
            lp_c = R._normal_logp(d["actions"][:, 1:].double(), d["mean"].double(), d["std"].double())
            for lp, old in ((lp_d, d["old_logp_d"]), (lp_c, d["old_logp_c"])):
                counts, away = R.surrogate_census(lp, old, d["advantages"], R.CLIP)
                assert len(counts) == 9 and min(counts.values()) > 0 and away > 1e-4, counts
            vc, d_clip, _ = R.value_census(d["value"], d["target_values"], d["returns"], R.CLIP)
            assert min(vc.values()) > 0 and d_clip > 1e-5, vc
    # the finish kernel's 11 lanes: 11 blocks, 12 (lane 0 twice)
    assert sorted(blocks) == [1, 2, 11, 12] and R.HYB_LANES == 11 and all(v == {0, 1} for v in blocks.values())
    assert [R.ppo_blocks(B) for B in R.HYB_B] == [1, 1, 1, 2, 11, 12]


@pytest.mark.parametrize("logits_form", [False, True])
def test_disc_loss_edges(be, logits_form):
    seen = []
    for i, sizes in enumerate(R.DISC_SIZES):
        (o, x), (again, _) = R.run_disc(be, sizes, logits_form, 8200 + i), R.run_disc(be, sizes, logits_form, 8200 + i)
        rows, (b_lb, b_pi, b_ulb) = sum(sizes), sizes
        assert o.nbytes == 4 * (R.DISC_SUMS + 1) * R.disc_blocks(rows), sizes
        _both_sides(R.disc_close(o), sizes)
        assert all(R.same_bits(getattr(o, k), getattr(again, k)) for k in ("out", "gd", "geps", "gc")), sizes
        assert float(o.geps[b_lb]) == 0.0 and float(x["eps"][b_lb]) == float(x["pol_eps"][0])                # de == 0: sign 0
        assert bool((o.geps[:b_lb] == 0).all()) and bool((o.geps[b_lb + b_pi:] == 0).all()) and bool((o.gd[:b_lb] == 0).all())
        # the argmax ties (classes 1 and 3 share the maximum in the first row of each segment, and in the first policy latent): the first index wins, as
        # torch.argmax -- the label of row 0 is 1, so acc_lb counts it only then; the reference's accuracies are compared above
        probs = torch.softmax(x["c"], -1) if logits_form else x["c"]
        assert float(probs[0, 1]) == float(probs[0, 3]) == float(probs[0].max()) and int(x["label"][0]) == 1 and float(x["pol_c"][0, 1]) == float(x["pol_c"][0, 3])
        if b_lb == 1:
            assert float(o.out[5]) == 1.0
        if b_pi == 1:
            assert float(o.out[8]) == 1.0
        if logits_form:
            assert float(probs[-1, 1]) == 1.0 and float(probs[-1].min()) < R.DISC_CLAMP                     # the saturated row: four classes under the clamp
        else:
            assert float(x["c"][0, 4]) == 0.0 == float(x["c"][-1, 0]) and float(o.gc[0, 4]) == 0.0 == float(o.gc[-1, 0])      # exactly 0: clamped, no gradient
        seen.append((R.disc_blocks(rows), R.disc_segments(sizes)))
    assert [nb for nb, _ in seen] == [1, 1, 1, 2, 2, 3]
    # where the three segments change: inside one wavefront (rows 1 and 2), on a wavefront's edge (64, 128), at a block's last lane and first (255 | 256), with the
    # third segment alone in the second block (200, 256 | 257 rows), and one row into the first block's first wave (1, then 256 = a block edge)
    assert [s for _, s in seen] == [[(0, 1), (0, 2)], [(0, 63), (1, 0)], [(1, 0), (2, 0)], [(3, 63), (4, 0)], [(3, 8), (4, 0)], [(0, 1), (4, 0)]]
