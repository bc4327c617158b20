"""Host side of the LightControl training step (x2i_amd/lightcontrol_step.py): the documented semantics of the noising kernel as a torch
expression, and the reference's timestep sampling / sigma lookup (lightcontrol/train_lightcontrol.py:412-420, :693-714, :756)."""
import torch

from oracle import sampler as OS
from tests.util import seeded
from x2i_amd.lightcontrol_step import flow_match_noise_reference, sample_timesteps, sigmas_for
from x2i_amd.pipeline import FlowMatchEulerDiscreteScheduler


def _dev_scheduler():
    return FlowMatchEulerDiscreteScheduler(shift=3.0, use_dynamic_shifting=True)   # FLUX.1-dev: the training tables are unshifted


def test_noising_formula_known_answers_and_packing():
    for dtype in (torch.float32, torch.bfloat16):
        x, n = seeded((3, 16, 12, 20), 1).to(dtype), seeded((3, 16, 12, 20), 2).to(dtype)
        y0, t0 = flow_match_noise_reference(x, n, torch.zeros(3))
        y1, t1 = flow_match_noise_reference(x, n, torch.ones(3))
        assert y0.shape == (3, 60, 64) and t0.shape == (3, 60, 64)
        assert torch.equal(y0, OS.pack_latents(x))                       # sigma = 0: the packed latents
        assert torch.equal(y1, OS.pack_latents(n))                       # sigma = 1: the packed noise
        assert torch.equal(t0, OS.pack_latents(n - x)) and torch.equal(t1, t0)
    # the layout, element by element: packed[b, i (w/2) + j, 4c + 2dy + dx] = t[b, c, 2i + dy, 2j + dx]
    x = torch.arange(2 * 4 * 4 * 6, dtype=torch.float32).reshape(2, 4, 4, 6)
    y, _ = flow_match_noise_reference(x, torch.zeros_like(x), torch.zeros(2))
    for b, c, i, j, dy, dx in [(0, 0, 0, 0, 0, 0), (1, 3, 1, 2, 1, 0), (0, 2, 1, 1, 0, 1), (1, 1, 0, 2, 1, 1)]:
        assert y[b, i * 3 + j, 4 * c + 2 * dy + dx] == x[b, c, 2 * i + dy, 2 * j + dx]
    # per-sample sigmas, and in bf16 every operation rounds (the kernel's contract)
    xb, nb = seeded((2, 16, 4, 4), 3).bfloat16(), seeded((2, 16, 4, 4), 4).bfloat16()
    sig = torch.tensor([0.3, 0.7])
    yb, _ = flow_match_noise_reference(xb, nb, sig)
    s = sig.bfloat16().float().reshape(2, 1, 1, 1)
    a = (1.0 - s).bfloat16().float()
    want = ((a * xb.float()).bfloat16().float() + (s * nb.float()).bfloat16().float()).bfloat16()
    assert torch.equal(yb, OS.pack_latents(want))


def test_timestep_sampling_and_sigma_lookup():
    sch = _dev_scheduler()
    ts = sample_timesteps(sch, 64, torch.Generator().manual_seed(5))
    assert ts.shape == (64,) and ts.dtype == torch.float32
    assert all(bool((sch.timesteps == t).any()) for t in ts)            # members of the table
    assert len(set(ts.tolist())) > 16                                   # one draw per image
    assert torch.equal(ts, sample_timesteps(sch, 64, torch.Generator().manual_seed(5)))
    assert not torch.equal(ts, sample_timesteps(sch, 64, torch.Generator().manual_seed(6)))
    # the statements of :693-701 on the same generator
    g = torch.Generator().manual_seed(5)
    u = torch.sigmoid(torch.randn((64,), generator=g))
    assert torch.equal(ts, sch.timesteps[(u * sch.config.num_train_timesteps).long()])
    sig = sigmas_for(sch, ts)
    assert sig.dtype == torch.float32 and torch.equal(sig, ts / 1000)   # unshifted table: sigma = t / 1000
    assert torch.equal(sig, sigmas_for(sch, ts))
    # a shifted table (schnell-style static shift) is looked up, not recomputed
    sh = FlowMatchEulerDiscreteScheduler(shift=3.0)
    t2 = sample_timesteps(sh, 8, torch.Generator().manual_seed(7))
    s2 = sigmas_for(sh, t2)
    assert torch.allclose(s2, t2 / 1000, rtol=1e-6) and all(bool((sh.sigmas == v).any()) for v in s2)
