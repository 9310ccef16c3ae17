"""The inputs of tests/golden/learner_steps.pt's steps, drawn here from a fixed seed instead of stored in the fixture (they were most of its size).
tools/gen_golden.py gen_learner_steps feeds exactly these tensors to the reference and stores their SHA-256; the tests redraw them and
check the digest first, so the comparison never silently runs on other inputs (a changed torch generator fails loudly there)."""
import hashlib

import torch

SEED = 2024
PPO_ROWS = (96, 96, 96, 37)
DISC_ROWS = (96, 96, 96)


def _ppo_sample(g, B):
    """(obs, actions, target_values, advantages, returns, old_logp, old_mu, old_sigma); the step's critic_obs IS obs"""
    obs = torch.randn(B, 671, generator=g) * 0.5
    obs[:, 666:671] = torch.nn.functional.one_hot(torch.randint(0, 5, (B,), generator=g), 5).float()
    obs[:, 665] = torch.rand(B, generator=g) * 2 - 1
    actions = torch.randn(B, 12, generator=g)
    old_mu = torch.randn(B, 12, generator=g) * 0.2
    old_sigma = torch.ones(B, 12) * (0.8 + 0.3 * torch.rand(B, 1, generator=g))
    return [obs, actions, torch.randn(B, 1, generator=g), torch.randn(B, 1, generator=g), torch.randn(B, 1, generator=g),
            torch.randn(B, 1, generator=g) - 12.0, old_mu, old_sigma]


def _disc_sample(g, B):
    """{"policy": (state, eps, one-hot c), "lb": (state, label), "ulb": state}"""
    pol = [torch.randn(B, 98, generator=g) * 1.3 + 0.2, torch.rand(B, 1, generator=g) * 2 - 1,
           torch.nn.functional.one_hot(torch.randint(0, 5, (B,), generator=g), 5).float()]
    lb = [torch.randn(B, 98, generator=g), torch.randint(0, 5, (B,), generator=g)]
    return {"policy": pol, "lb": lb, "ulb": torch.randn(B, 98, generator=g) * 0.8 - 0.1}


def samples():
    """(PPO samples, discriminator samples), in the order the generator draws them"""
    g = torch.Generator().manual_seed(SEED)
    ppo = [_ppo_sample(g, b) for b in PPO_ROWS]
    disc = [_disc_sample(g, b) for b in DISC_ROWS]
    return ppo, disc


def digest(ppo, disc):
    h = hashlib.sha256()
    for t in [t for s in ppo for t in s] + [t for s in disc for t in s["policy"] + s["lb"] + [s["ulb"]]]:
        h.update(str(tuple(t.shape)).encode()); h.update(str(t.dtype).encode()); h.update(t.contiguous().numpy().tobytes())
    return h.hexdigest()
