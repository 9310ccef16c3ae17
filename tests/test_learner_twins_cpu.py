"""CPU: the oracle's plain-C twins of the small learner kernels (qo_pair_loss, qo_gather_rows, qo_kl_lr_rule, qo_rollout_post_amp)
against the PyTorch expressions of the reference they restate.  The HIP kernels are held to the same expressions AND to these
twins in tests/test_fused_learner.py (-m gpu)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.oracle_lib import load_oracle

P = lambda a: C.c_void_p(a.ctypes.data)


@pytest.mark.parametrize("mode,rows,cols", [(0, 1000, 29), (1, 257, 4), (0, 1, 3)])
def test_pair_loss_twin(mode, rows, cols):
    """gail.py:346-358: mean row L2 norm of (a - b) / mean squared difference, value and gradient"""
    qo = load_oracle()
    torch.manual_seed(mode + cols)
    a0, wide = torch.randn(rows, cols), torch.randn(rows, cols + 7)
    if rows > 2:
        wide[2, 3:3 + cols] = a0[2]
    b0 = wide[:, 3:3 + cols]
    ra = a0.clone().requires_grad_(True)
    ref = (ra - b0).norm(p=2, dim=1).mean() if mode == 0 else (ra - b0).pow(2).mean()
    ref.backward()
    g, out = np.zeros((rows, cols), np.float32), np.zeros(1, np.float32)
    an, wn = np.ascontiguousarray(a0.numpy()), np.ascontiguousarray(wide.numpy())
    assert qo.qo_pair_loss(P(an), C.c_void_p(wn.ctypes.data + 12), rows, cols, cols + 7, mode, P(g), P(out), None, 0, None) == 0
    assert abs(out[0] - float(ref)) <= 2e-6 * max(1.0, abs(float(ref)))
    np.testing.assert_allclose(g, ra.grad.numpy(), rtol=2e-5, atol=1e-9)


def test_gather_rows_twin_plain_and_block_form():
    """rollout_storage.py:122-157: indexed reads of a minibatch; block form = row block of a (blocks, rows) index table"""
    qo = load_oracle()
    rng = np.random.default_rng(0)
    n, rows, blocks = 500, 64, 5
    srcs = [rng.normal(size=(n, w)).astype(np.float32) for w in (671, 12, 1, 29)]
    table = rng.integers(0, n, size=(blocks, rows)).astype(np.int64)
    k = len(srcs)
    sp = (C.c_void_p * k)(*[s.ctypes.data for s in srcs]); st = (C.c_int64 * k)(*[s.shape[1] for s in srcs]); wd = (C.c_int32 * k)(*[s.shape[1] for s in srcs])
    for blk in (None, 3):
        dsts = [np.zeros((rows, s.shape[1]), np.float32) for s in srcs]
        dp = (C.c_void_p * k)(*[d.ctypes.data for d in dsts])
        b = np.array([blk if blk is not None else 0], np.int64)
        assert qo.qo_gather_rows(P(table), P(b) if blk is not None else None, rows, k, sp, st, wd, dp, None) == 0
        idx = table[blk if blk is not None else 0]
        for d, s in zip(dsts, srcs):
            assert np.array_equal(d, s[idx])


def test_kl_lr_rule_twin():
    """gail.py:367-379"""
    qo = load_oracle()
    for kl, lr0 in [(0.05, 1e-3), (0.004, 1e-3), (0.01, 1e-3), (0.0, 1e-3), (-1.0, 1e-3), (0.05, 1.2e-5), (0.001, 9e-3)]:
        want = max(1e-5, lr0 / 1.5) if kl > 0.02 else (min(1e-2, lr0 * 1.5) if 0.0 < kl < 0.005 else lr0)
        hk, hl = np.array([kl], np.float32), np.array([lr0], np.float32)
        assert qo.qo_kl_lr_rule(P(hk), 0.01, 1.5, 1e-5, 1e-2, P(hl), None) == 0
        assert abs(float(hl[0]) - want) <= 1e-6 * want


def test_rollout_post_amp_twin():
    """discriminator.py:88-118 (MSELoss mapping) + the time-out bootstrap and episode sums of the runner"""
    qo = load_oracle()
    torch.manual_seed(7)
    n, dim_c, num_obs, stride = 300, 5, 671, 680
    obs = torch.randn(n, stride)
    rew, values, d, eps, logits = torch.rand(n), torch.randn(n), torch.randn(n) * 1.5 + 0.5, torch.randn(n), torch.randn(n, dim_c) * 2
    reset = (torch.rand(n) < 0.2).long(); tout = ((torch.rand(n) < 0.5) & (reset > 0)).to(torch.uint8)
    cur = torch.randn(6, n)
    ci, cus, css, ct, dt, gamma = 0.35, 0.1, 0.25, 0.3, 0.02, 0.99
    label_eps = obs[:, num_obs - dim_c - 1]
    label_c = F.one_hot(torch.argmax(obs[:, num_obs - dim_c:num_obs], dim=-1), num_classes=dim_c).float()
    c = torch.clamp(torch.softmax(logits, -1), 1e-20, torch.inf)
    r_i = torch.clamp(1 - 0.25 * torch.square(d - 1), min=0) * dt
    r_us = -torch.abs(eps - label_eps) * dt
    r_ss = -F.cross_entropy(c, label_c, reduction="none") * dt
    total = ci * r_i + cus * r_us + css * r_ss + ct * rew
    a = [np.ascontiguousarray(x.numpy()) for x in (rew, reset, tout, values, d, eps, logits, obs)]
    st_r, st_d = np.zeros(n, np.float32), np.zeros(n, np.uint8)
    cur_n, fin, mask = cur.numpy().copy(), np.zeros((6, n), np.float32), np.zeros(n, np.uint8)
    assert qo.qo_rollout_post_amp(*[P(x) for x in a[:7]], dim_c, P(a[7]), stride, num_obs, ci, cus, css, ct, dt, gamma, n,
                                  P(st_r), P(st_d), P(cur_n), P(fin), P(mask), None) == 0
    np.testing.assert_allclose(st_r, (total + gamma * values * tout.float()).numpy(), rtol=2e-5, atol=2e-6)
    want_fin = cur + torch.stack([total, r_i, r_us, r_ss, rew, torch.ones(n)])
    np.testing.assert_allclose(fin, want_fin.numpy(), rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(cur_n, (want_fin * (reset == 0)).numpy(), rtol=2e-5, atol=2e-6)
    assert np.array_equal(st_d, (reset > 0).numpy().astype(np.uint8)) and np.array_equal(mask, st_d)


def test_hybrid_ppo_loss_twin_matches_the_eager_objective_and_its_autograd_gradient():
    """qo_hybrid_ppo_loss (the C twin the HIP kernel is checked against) vs the task-level update's own eager expression
    (tsc/rsl_rl/algorithms/ppo.py:222-262 through torch.distributions and autograd): every loss term and all four gradients"""
    import ctypes as C
    import torch
    from torch.distributions import Categorical, Normal
    from tests.oracle_lib import load_oracle
    lib = load_oracle()
    f = lib.qo_hybrid_ppo_loss
    torch.manual_seed(3)
    B, ND, NC, clip, cv, ce = 777, 3, 18, 0.2, 1.0, 0.01
    logits = (torch.randn(B, ND) * 2).requires_grad_(True)
    mean = torch.randn(B, NC).requires_grad_(True)
    std = (torch.rand(NC) * 0.8 + 0.3).requires_grad_(True)
    value = torch.randn(B).requires_grad_(True)
    a_d = torch.randint(0, ND, (B,))
    actions = torch.cat([a_d.float().unsqueeze(1), mean.detach() + torch.randn(B, NC) * 0.7], 1)
    old_mu, old_sigma = mean.detach() + 0.1 * torch.randn(B, NC), (std.detach() * (1 + 0.1 * torch.randn(NC))).abs().expand(B, NC).contiguous()
    old_logp_d = torch.log_softmax(logits.detach() + 0.3 * torch.randn(B, ND), -1)[torch.arange(B), a_d]
    old_logp_c = Normal(old_mu, old_sigma).log_prob(actions[:, 1:]).sum(-1) + 0.2 * torch.randn(B)
    adv, ret, tv = torch.randn(B), torch.randn(B), value.detach() + 0.3 * torch.randn(B)
    # eager expression
    dist_d = Categorical(probs=torch.softmax(logits, -1), validate_args=False)
    dist_c = Normal(mean, mean * 0.0 + std, validate_args=False)
    logp_d, logp_c = dist_d.log_prob(a_d.float()), dist_c.log_prob(actions[:, 1:]).sum(-1)
    ent = dist_c.entropy().mean(-1) + dist_d.entropy()
    surr = lambda lp, olp: torch.max(-adv * torch.exp(lp - olp), -adv * torch.clamp(torch.exp(lp - olp), 1 - clip, 1 + clip)).mean()   # noqa: E731
    s_d, s_c = surr(logp_d, old_logp_d), surr(logp_c, old_logp_c)
    vclip = tv + (value - tv).clamp(-clip, clip)
    vl = torch.max((value - ret).pow(2), (vclip - ret).pow(2)).mean()
    loss = s_d + s_c + cv * vl - ce * ent.mean()
    loss.backward()
    sigma = dist_c.stddev
    kl = torch.sum(torch.log(sigma / old_sigma + 1e-5) + (old_sigma.square() + (old_mu - mean).square()) / (2 * sigma.square()) - 0.5, -1).mean()
    # twin
    c = lambda t: t.detach().contiguous()                                    # noqa: E731
    ins = [c(x) for x in (logits, mean, std, value, actions, old_logp_d, old_logp_c, old_mu, old_sigma, adv, ret, tv)]
    dlg, dmu, dsd, dv, out = torch.empty(B, ND), torch.empty(B, NC), torch.empty(NC), torch.empty(B), torch.empty(8)
    assert f(*[t.data_ptr() for t in ins], B, ND, NC, clip, cv, ce, 1, dlg.data_ptr(), dmu.data_ptr(), dsd.data_ptr(), dv.data_ptr(), out.data_ptr(), None, 0, None) == 0
    ref = [loss.item(), (s_d + s_c).item(), vl.item(), ent.mean().item(), kl.item(), s_d.item(), s_c.item()]
    assert np.allclose(out.numpy()[:7], ref, rtol=2e-5, atol=2e-6), (out, ref)
    for got, want, name in ((dlg, logits.grad, "logits"), (dmu, mean.grad, "mean"), (dsd, std.grad, "std"), (dv, value.grad, "value")):
        assert torch.allclose(got, want, rtol=2e-4, atol=2e-7), (name, (got - want).abs().max())


def test_penalty_chain_through_proxy_leaves_gives_the_same_gradients():
    """Discriminator.forward_with_input_gradient(proxies=[...]): the gradient-penalty chain reads the weights through leaves that share
    their storage, and the caller adds proxy.grad to param.grad -- the same two addends per weight as autograd's own accumulation, so
    heads, input gradient and every parameter gradient are bit-identical to the direct form (CPU: the fused helpers fall back to torch)."""
    import torch
    from quadrupedal_agility_amd.rsl_rl.algorithms.discriminator import Discriminator

    class Env:
        task_obs_weight_decay, task_obs_weight = False, 1.0
    torch.manual_seed(1)
    d = Discriminator(Env(), 98, 49, 5, 0.02, "MSELoss", None, 1.0, 0.01, 0.2, 0.2, 2, 2, 0.0, [64, 32], "cpu")
    x = torch.randn(60, 98)
    rows = slice(40, None)
    seeds = [torch.randn(60, 1), torch.randn(60, 1), torch.randn(60, 5), torch.randn(20, 98)]
    out = []
    for use_proxies in (False, True):
        d.zero_grad(set_to_none=True)
        proxies = [] if use_proxies else None
        (dl, eps, c), g = d.forward_with_input_gradient(x, rows, clamp=False, proxies=proxies)
        torch.autograd.backward([dl, eps, c, g], seeds)
        if use_proxies:
            assert len(proxies) == 3 and all(q.data_ptr() == w.data_ptr() for w, q in proxies)
            for w, q in proxies:
                w.grad.add_(q.grad)
        out.append(([t.detach().clone() for t in (dl, eps, c, g)], [p.grad.clone() for p in d.parameters()]))
    for a, b in zip(out[0][0] + out[0][1], out[1][0] + out[1][1]):
        assert torch.allclose(a, b, rtol=1e-6, atol=1e-7)


def test_data_parallel_normaliser_moments_match_the_single_process_update_for_offset_features():
    """Normalizer.batch_moments / update_from_batch_moments (the discriminator-input normaliser under data parallelism): two
    ranks' fp32 bucket entries must reproduce the one-process RunningMeanStd.update (bbc/rsl_rl/utils/utils.py:62-84, double) also for
    features whose mean is large against their spread -- raw E[x], E[x^2] in fp32 lose the variance there"""
    import numpy as np
    import torch
    from quadrupedal_agility_amd.rsl_rl.utils.utils import TorchNormalizer
    g = torch.Generator().manual_seed(0)
    dim = 6
    offset = torch.tensor([0.0, 1.0, 50.0, -300.0, 1000.0, 3.0])
    spread = torch.tensor([1.0, 0.1, 0.05, 0.2, 0.5, 2.0])
    single, dp = TorchNormalizer(dim, "cpu"), TorchNormalizer(dim, "cpu")
    for step in range(8):
        halves = [(torch.randn(614, dim, generator=g) * spread + offset).float() for _ in range(2)]        # the two ranks' rows of one batch
        single.update_torch([torch.cat(halves)])
        if dp.cold():            # first folds: raw moments, fp64 collective
            moments = torch.stack([dp.batch_moments_exact([h]) for h in halves]).mean(0)
            assert moments.dtype == torch.float64
        else:                    # then: about the running mean, in the fp32 gradient bucket
            moments = torch.stack([dp.batch_moments([h]) for h in halves]).mean(0)
            assert moments.dtype == torch.float32
        dp.update_from_batch_moments(moments, [1228])
    assert not dp.cold()
    np.testing.assert_allclose(dp.mean.numpy(), single.mean.numpy(), rtol=1e-7, atol=1e-7)
    np.testing.assert_allclose(dp.var.numpy(), single.var.numpy(), rtol=1e-6)
    # the raw fp32 moments this replaces: 2 % off on the feature with mean 1000 and spread 0.5
    h = (torch.randn(1228, dim, generator=g) * spread + offset).float().double()
    raw = torch.stack([h.mean(0), h.square().mean(0)]).float().double()
    assert abs(float((raw[1] - raw[0] ** 2)[4] / h.var(0, unbiased=False)[4]) - 1.0) > 1e-3
