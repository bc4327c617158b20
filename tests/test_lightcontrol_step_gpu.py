"""The LightControl training step on the HIP path (x2i_amd/lightcontrol_step.py; lightcontrol/train_lightcontrol.py:672-775): the two kernels of
its head (flow-matching noising, MSE loss + gradient), the transformer's activation-gradient chain seeded at the loss and read at the control
injections, the whole step's control-net gradients against float64 autograd through the oracle, and the step's behaviour."""
import math

import pytest
import torch

from oracle import flux as OF
from oracle import sampler as OS
from tests.util import rel_l2, seeded

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24


def bf(x):
    return x.to(torch.bfloat16)


def rb(x):
    return x.to(torch.bfloat16).float()


def bits(x):
    return x.detach().cpu().contiguous().view(torch.int16)


# -------------------------------------------------------------------------------------------------------------- 1. noising kernel
# one token; odd-sized (w % 8 != 0: the 4-byte path; 3 x 6 x 10 x 8 = 1440 work items, no multiple of a workgroup); w % 8 == 0 (16-byte path)
@pytest.mark.parametrize("B,C,h,w", [(1, 16, 2, 2), (3, 16, 12, 20), (2, 16, 16, 16)])
def test_noise_kernel_is_bit_identical_to_the_torch_bf16_expression(B, C, h, w):
    from x2i_amd import ops
    from x2i_amd.lightcontrol_step import flow_match_noise_reference
    x, n = bf(seeded((B, C, h, w), 1)), bf(seeded((B, C, h, w), 2))
    pool = [0.0, 1.0, 0.3, 0.7373, 0.999]          # 0, 1, and values that are no bf16 numbers
    for rot in range(len(pool)):
        sig = torch.tensor([pool[(rot + b) % len(pool)] for b in range(B)])
        want_y, want_t = flow_match_noise_reference(x, n, sig)          # torch on bf16 tensors, then the project's _pack_latents
        got_y, got_t = ops.flow_match_noise(x.to(DEV), n.to(DEV), sig.to(DEV))
        assert got_y.shape == (B, (h // 2) * (w // 2), 4 * C)
        assert torch.equal(bits(got_y), bits(want_y)), (rot, sig)
        assert torch.equal(bits(got_t), bits(want_t)), (rot, sig)
        assert torch.equal(got_y.cpu(), OS.pack_latents((1.0 - bf(sig).view(B, 1, 1, 1)) * x + bf(sig).view(B, 1, 1, 1) * n))


# -------------------------------------------------------------------------------------------------------------- 2. loss kernel
def _mse_chain_terms(n):
    """Roundings between a term (pred - target)^2 and the scalar, from the summation order of x2i_mse_loss_grad_bf16 + x2i_reduce_rows_f32
    (csrc/train.hip): the difference (counted twice: it is squared); one fmaf per element of a thread's chain, a thread owning every 256th
    8-element vector of its workgroup's share; six DPP steps of the wave sum; three adds over the four waves; then reduce_rows over the nb
    partials: a wave's chain over every 16th partial, three levels over its eight accumulators, sixteen waves added in order, the multiply
    by 1 / n."""
    from x2i_amd import ops
    nb = ops.mse_loss_workspace_floats(n)
    per_block = math.ceil(n // 8 / nb)
    return 2 + 8 * math.ceil(per_block / 256) + 6 + 3 + (math.ceil(nb / 16) + 3 + 16 + 1), nb


@pytest.mark.parametrize("B,Si", [(1, 1), (3, 60), (2, 4096)])      # one vector row; three ragged workgroups; 128 workgroups of 512 vectors
def test_loss_kernel_against_float64(B, Si):
    from x2i_amd import ops
    pred, target = bf(seeded((B, Si, 64), 3)), bf(seeded((B, Si, 64), 4, 0.8))
    n = pred.numel()
    diff = pred.double() - target.double()
    loss64 = (diff ** 2).mean().item()
    terms, nb = _mse_chain_terms(n)
    loss, d = ops.mse_loss_grad(pred.to(DEV), target.to(DEV))
    assert loss.dtype == torch.float32 and d.dtype == torch.bfloat16 and d.shape == pred.shape
    # every term is >= 0, so sum |terms| = n * loss64
    err, bound = abs(loss.double().item() - loss64), terms * U * loss64
    print(f"mse loss [{B}, {Si}, 64]: {nb} workgroups, {terms} roundings, |loss - loss64| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    # gradient: bf16 rounding of a value computed in f32
    d64 = 2.0 * diff / n
    assert bool(((d.double().cpu() - d64).abs() <= 2.0 ** -8 * d64.abs()).all())
    # no atomics: a second launch is bit-identical
    loss2, d2 = ops.mse_loss_grad(pred.to(DEV), target.to(DEV))
    assert torch.equal(loss, loss2) and torch.equal(bits(d), bits(d2))
    # grad_scale = 0.5 halves the gradient exactly and leaves the loss alone
    loss3, d3 = ops.mse_loss_grad(pred.to(DEV), target.to(DEV), grad_scale=0.5)
    assert torch.equal(loss, loss3) and torch.equal(d3.float() * 2, d.float())


# -------------------------------------------------------------------------------------------------------------- 3. chain to the injections
def _tiny():
    """(the helper of tests/test_train_gpu.py, with the guidance embedder of FLUX.1-dev)"""
    from x2i_amd.flux import FluxTransformer2DModel
    cfg = dict(OF.DEFAULT_CFG)
    cfg.update(num_layers=2, num_single_layers=2, num_attention_heads=2, joint_attention_dim=64, pooled_projection_dim=32, guidance_embeds=True)
    sd = OF.random_flux_state_dict(cfg, seed=11, std=0.05)
    m = FluxTransformer2DModel(**cfg, device=DEV)
    m.load_state_dict({k: v.bfloat16() for k, v in sd.items()}, strict=True)
    return m, {k: v.bfloat16().float() for k, v in sd.items()}, cfg


def _oracle_guidance(B, scale=3.5):
    """the model forms guidance * 1000 in bf16 (lightcontrol_flux.py:449: 3500 -> 3504); the oracle gets the value that gives the same product"""
    return (torch.full((B,), scale).bfloat16() * 1000).float() / 1000


def test_chain_seeded_at_the_loss_gives_the_gradient_at_both_injections(monkeypatch):
    """2 + 2 blocks, D = 256, 24 text + 8 x 8 image tokens, B = 2 with two timesteps, a random d noise_pred and two fixed random control outputs
    added behind the double blocks: d loss / d control output i as on_injection sees it, against autograd through the f32 oracle on the same
    bf16-rounded weights (the oracle's control nets are replaced by the fixed tensors).  rel-L2 bound 2.5e-2: the bound tests/test_train_gpu.py
    sets for this chain."""
    from x2i_amd.lightcontrol_step import add_control_outputs
    from x2i_amd.train import DistillBackward
    m, sd, cfg = _tiny()
    B, St, h2, w2, D = 2, 24, 8, 8, 256
    Si = h2 * w2
    gen = torch.Generator().manual_seed(0)
    hid = torch.randn((B, Si, 64), generator=gen).bfloat16()
    enc, pooled = torch.randn((B, St, 64), generator=gen).bfloat16(), torch.randn((B, 32), generator=gen).bfloat16()
    ts = torch.tensor([0.5, 0.25])                       # t * 1000 is exact in bf16, as the f32 oracle sees it
    ids, tids = OS.prepare_latent_image_ids(h2, w2), torch.zeros(St, 3)
    seed = (torch.randn((B, Si, 64), generator=gen) * 0.05).bfloat16()
    ctrl = [(torch.randn((B, Si, D), generator=gen) * 0.5).bfloat16() for _ in range(2)]
    # oracle: controlnext_forward stands in for "add this tensor"
    leaves = [c.float().transpose(1, 2).reshape(B, D, h2, w2).clone().requires_grad_(True) for c in ctrl]
    monkeypatch.setattr(OF, "controlnext_forward", lambda csd, prefix, hint, t: {"out": leaves[csd["index"]], "scale": 1.0})
    ref_out = OF.flux_forward(sd, cfg, hid.float(), enc.float(), pooled.float(), ts, ids, tids, guidance=_oracle_guidance(B), guided_hint=None,
                              control_sds=[{"index": 0}, {"index": 1}])
    (ref_out * seed.float()).sum().backward()
    want = [leaf.grad.flatten(2).transpose(1, 2) for leaf in leaves]
    bw = DistillBackward(m)
    st = bw.prepare_conditioning(enc.to(DEV), pooled.to(DEV), tids.to(DEV), ids.to(DEV), torch.full((B,), 3.5, device=DEV))
    control = add_control_outputs([c.to(DEV) for c in ctrl])
    out, _ = bw.forward_train(st, hid.to(DEV), ts.to(DEV), control=control, keep_head=True)
    assert bw.saved["injections"] == 2
    assert rel_l2(out, ref_out.detach()) < 2e-2
    # the saving forward with the injections is the sampling forward with them
    assert rel_l2(out, m.denoise(st, hid.to(DEV), ts.to(DEV), control=control)) < 1e-2
    full, order = {}, []

    def grab(store):
        def on_injection(i, dX, St_, S_, D_):
            assert (St_, S_, D_) == (St, St + Si, D) and tuple(dX.shape) == (B, St + Si, D)
            store[i] = dX[:, St_:].clone()
            order.append(i)
        return on_injection
    d_enc, d_pooled = bw.backward(seed=seed.to(DEV), on_injection=grab(full))
    assert order == [1, 0] and d_enc.shape == (B, St, 64) and d_pooled.shape == (B, 32)
    for i in range(2):
        e = rel_l2(full[i], want[i])
        print(f"d loss / d control output {i} (chain seeded at d noise_pred, 2+2 blocks): rel-L2 {e:.3e}")
        assert e < 2.5e-2   # measured 4.4e-3 / 3.6e-3
    # stopping behind injection 0 changes nothing above it
    stopped = {}
    bw.forward_train(st, hid.to(DEV), ts.to(DEV), control=control, keep_head=True)
    assert bw.backward(seed=seed.to(DEV), on_injection=grab(stopped), stop_after_injections=True) == (None, None)
    assert all(torch.equal(bits(stopped[i]), bits(full[i])) for i in range(2))


# -------------------------------------------------------------------------------------------------------------- 4-6. the whole step
def _nets(n, seed, out_channels):
    from x2i_amd.lightcontrol import ControlNeXtModel
    nets, sds = [], []
    for i in range(n):
        sd = OF.random_controlnext_state_dict(seed=seed + i, out_channels=out_channels)
        net = ControlNeXtModel(device=DEV, control_out_channels=out_channels)
        net.load_state_dict({k: bf(v) for k, v in sd.items()}, strict=True)
        nets.append(net)
        sds.append({k: rb(v) for k, v in sd.items()})
    return nets, sds


def _batch(B, St, joint, pooled_dim, h, w, seed=40):
    """A training batch with per-sample timesteps whose /1000, x1000 round trip is exact in bf16 (500, 250: the f64 oracle then sees the values the
    bf16 model forms, lightcontrol_flux.py:447) and the dev table's sigmas for them."""
    from x2i_amd.lightcontrol_step import sigmas_for
    from x2i_amd.pipeline import FlowMatchEulerDiscreteScheduler
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=gen)  # noqa: E731
    timesteps = torch.tensor([500.0, 250.0][:B])
    return dict(latents=bf(rn(B, 16, h, w)), noise=bf(rn(B, 16, h, w)), timesteps=timesteps,
                sigmas=sigmas_for(FlowMatchEulerDiscreteScheduler(shift=3.0, use_dynamic_shifting=True), timesteps),
                prompt_embeds=bf(rn(B, St, joint)), pooled_prompt_embeds=bf(rn(B, pooled_dim)),
                guided_hint=rb(torch.rand((B, 3, 8 * h, 8 * w), generator=gen) * 2 - 1))


def _oracle_step_grads(sd, cfg, csds, batch, dtype):
    """Control-net gradients and loss of the reference's step in `dtype`: oracle transformer with the control nets behind its double blocks
    (flux_forward(control_sds=...)), the loss expression of train_lightcontrol.py:758-762 on the packed rows (unpacking is a permutation)."""
    from x2i_amd.lightcontrol_step import flow_match_noise_reference
    B, _, h, w = batch["latents"].shape
    noisy, target = flow_match_noise_reference(batch["latents"], batch["noise"], batch["sigmas"])     # bf16, as the reference forms them
    params = [{k: v.to(dtype).requires_grad_() for k, v in c.items()} for c in csds]
    sdd = {k: v.to(dtype) for k, v in sd.items()}
    pred = OF.flux_forward(sdd, cfg, noisy.to(dtype), batch["prompt_embeds"].to(dtype), batch["pooled_prompt_embeds"].to(dtype),
                           (batch["timesteps"] / 1000).to(dtype), OS.prepare_latent_image_ids(h // 2, w // 2), torch.zeros(batch["prompt_embeds"].shape[1], 3),
                           guidance=_oracle_guidance(B), guided_hint=batch["guided_hint"].to(dtype), control_sds=params)
    acc = torch.float64 if dtype == torch.float64 else torch.float32
    loss = torch.mean(((pred.to(acc) - target.to(acc)) ** 2).reshape(B, -1), 1).mean()
    loss.backward()
    return [torch.cat([p[k].grad.double().reshape(-1) for k in c]) for p, c in zip(params, csds)], loss.item()


def _hip_net_grads(tr, csds):
    """per net, every parameter's gradient as one vector, in the key order of the oracle's state dict"""
    g = tr.named_grads()
    assert len(g) == sum(len(c) for c in csds)
    return [torch.cat([g["%d.%s" % (i, k)].double().reshape(-1).cpu() for k in c]) for i, c in enumerate(csds)]


def _check_step_gradients(m, sd, cfg, nets, csds, batch, what):
    from x2i_amd.lightcontrol_step import LightControlTrainStep
    from x2i_amd.lightcontrol_train import ControlNeXtTrainer
    tr = ControlNeXtTrainer(nets)
    step = LightControlTrainStep(m, tr)
    loss = step(**{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}, optimizer_step=False)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.device.type == "cuda"
    hip = _hip_net_grads(tr, csds)
    g64, loss64 = _oracle_step_grads(sd, cfg, csds, batch, torch.float64)
    try:
        g16, loss16 = _oracle_step_grads(sd, cfg, csds, {k: (bf(v) if k == "guided_hint" else v) for k, v in batch.items()}, torch.bfloat16)
    except RuntimeError as e:      # an op without a bf16 CPU kernel: the 2.5e-2 term alone (see the docstrings)
        print("bf16 oracle unavailable (%s): checking against the 2.5e-2 term alone" % str(e).splitlines()[0])
        g16, loss16 = None, float("nan")
    print(f"{what}: loss HIP {loss.item():.6f}  float64 {loss64:.6f}  bf16 oracle {loss16:.6f}")
    worst, bad = 0.0, []
    for i, (gh, gr) in enumerate(zip(hip, g64)):
        e_hip, nrm = (gh - gr).norm().item(), gr.norm().item()
        e_bf = (g16[i] - gr).norm().item() if g16 is not None else 0.0
        print(f"  net {i}: |g64| {nrm:.3e}  HIP error {e_hip:.3e} ({e_hip / nrm:.3e} rel)  bf16 oracle error {e_bf:.3e} ({e_bf / nrm:.3e} rel)")
        worst = max(worst, e_hip / max(e_bf, 1e-300))
        if not e_hip <= max(2.0 * e_bf, 2.5e-2 * nrm):
            bad.append(i)
    print(f"  worst HIP / bf16-oracle error ratio {worst:.3f}")
    assert not bad, bad
    assert abs(loss.item() - loss64) <= 1e-3 * abs(loss64)
    return tr, step


def test_whole_step_control_gradients_against_float64_autograd():
    """Tiny dev model (2 + 2 blocks, D = 256, guidance embedder), two control nets with 256 output channels on a 128 x 128 hint (8 x 8 tokens),
    B = 2 with per-sample timesteps.  Reference: float64 autograd through oracle.flux.flux_forward(control_sds=...) and the reference's loss
    expression; yardstick: the same oracle with bf16 parameters and activations under autograd, which is what the reference's training does.
    Per net, all parameters as one vector: HIP error <= max(2 x the bf16 oracle's error, 2.5e-2 |g64|) -- the factor 2 because two bf16 chains,
    the transformer's and the net's, compose; 2.5e-2 is the project's bound for the transformer chain.  Should the bf16 oracle meet an op
    without a CPU kernel, the 2.5e-2 term alone decides.  The loss agrees with float64 to 1e-3.  Measured: HIP 1.79e-2 / 2.38e-2 of |g64| (net 0 / 1), the bf16 oracle
    1.88e-2 / 2.55e-2; loss 2.768199 vs 2.768395."""
    m, sd, cfg = _tiny()
    nets, csds = _nets(2, seed=50, out_channels=256)
    _check_step_gradients(m, sd, cfg, nets, csds, _batch(2, 24, 64, 32, 16, 16), "tiny step")


def test_full_width_step_control_gradient_against_float64_autograd():
    """D = 3072, 24 heads, 1 + 1 blocks, 64 text + 8 x 8 image tokens, B = 1, one control net with 3072 output channels on a 128 x 128 hint: the
    row stride 3072 / offset St D addressing between the chain's dX and backward_net, which D = 256 cannot get wrong in the same way.  Same
    criterion as the tiny test.  Measured: HIP 2.53e-2 of |g64|, the bf16 oracle 2.77e-2; loss 3.266732 vs 3.266483."""
    from x2i_amd.flux import FluxTransformer2DModel
    cfg = dict(OF.DEFAULT_CFG)
    cfg.update(num_layers=1, num_single_layers=1, guidance_embeds=True)
    sd = OF.random_flux_state_dict(cfg, seed=21, std=0.02, dtype=torch.bfloat16)
    m = FluxTransformer2DModel(**cfg, device=DEV)
    m.load_state_dict(sd, strict=True)
    nets, csds = _nets(1, seed=60, out_channels=3072)
    _check_step_gradients(m, sd, cfg, nets, csds, _batch(1, 64, 4096, 768, 16, 16, seed=41), "full-width step")


def test_step_behaviour_optimizer_accumulation_descent_and_frozen_transformer():
    from x2i_amd.lightcontrol_step import LightControlTrainStep
    from x2i_amd.lightcontrol_train import ControlNeXtTrainer
    m, _, _ = _tiny()
    frozen = {k: v.clone() for k, v in m.state_dict().items()}
    nets, _ = _nets(2, seed=50, out_channels=256)
    tr = ControlNeXtTrainer(nets, lr=1e-3, max_grad_norm=0.5)
    step = LightControlTrainStep(m, tr)
    batch = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in _batch(2, 24, 64, 32, 16, 16).items()}
    # a zero seed gradient (grad_scale = 0) leaves every control gradient exactly zero
    step(**batch, optimizer_step=False, grad_scale=0.0)
    assert float(tr.grad.abs().max()) == 0.0
    # the step's own gradients
    loss0 = step(**batch, optimizer_step=False)
    grads = tr.grad.clone()
    assert bool(torch.isfinite(grads).all()) and float(grads.norm()) > 0
    # two half-scaled calls accumulate to them (a power-of-two scale goes through every bf16 rounding; the sums are f32)
    tr.zero_grad()
    for _ in range(2):
        step(**batch, optimizer_step=False, grad_scale=0.5)
    assert rel_l2(tr.grad, grads) < 1e-6
    # optimizer_step=True: clip_grad_norm_ + torch.optim.AdamW on those gradients (the comparison of tests/test_controlnext_train_gpu.py)
    tr.zero_grad()
    params = [p.detach().clone().requires_grad_() for p in tr.params]
    opt = torch.optim.AdamW(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    for p, n in zip(params, tr.names):
        o, s = tr.off[n]
        p.grad = grads[o:o + s].view(p.shape).to(torch.bfloat16)
    torch.nn.utils.clip_grad_norm_(params, 0.5)
    opt.step()
    loss1 = step(**batch, optimizer_step=True)
    assert torch.equal(loss0, loss1) and tr.step_count == 1 and float(tr.grad.abs().max()) == 0.0
    assert abs(tr.last_norm[1].item() - grads.norm().item()) <= 1e-4 * grads.norm().item()
    for p, q in zip(tr.params, params):
        assert (p.float() - q.float()).abs().max().item() <= 2 * (2.0 ** -8) * q.float().abs().max().item() + 1e-6
    # eight steps on the fixed batch lower the loss
    losses = [loss1.item()] + [step(**batch).item() for _ in range(8)]
    print("loss over repeated steps on one batch:", " ".join(f"{v:.5f}" for v in losses))
    assert losses[-1] < losses[0]
    # the transformer is frozen
    after = m.state_dict()
    assert frozen.keys() == after.keys() and all(torch.equal(bits(frozen[k]), bits(after[k])) for k in frozen)
