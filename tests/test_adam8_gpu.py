"""Block-wise 8-bit AdamW on the GPU (csrc/optim8.hip, x2i_amd/optim.py: FlatAdamW8bit, the trainers' use_8bit_adam): every launch against the
float64 reference and per-element checker of tests/adam8_ref.py, from the state the kernel read; what it must not touch; the optimizer class
against FlatAdamW; the two trainers and the training program with the option; and the default path, which must not have moved.

Parameter sets of the kernel tests (elements per parameter): 256, 255, 257, 4096 + 37, the three-parameter table (4096, 4352 + 5, 8192) whose
second parameter starts 6 bytes off an 8-byte boundary (the 2-byte parameter path), and GRID_STRIDE_N = 8192 * 256 + 3 * 256 + 5: the launch
has at most 2048 workgroups of four waves, one block per wave and pass, so blocks 8192.. are reached only by the grid stride."""
import math

import pytest
import torch

from tests import adam8_ref as R
from tests.gemm_ref import check_untouched, poison_, sentinel_bits, write_mask

pytestmark = pytest.mark.gpu
DEV = "cuda"
HYP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
SETS = {"256": [256], "255": [255], "257": [257], "4096+37": [4096 + 37], "three": [4096, 4352 + 5, 8192]}
GRID_STRIDE_N = 8192 * 256 + 3 * 256 + 5
# (clip coefficient, weight decay, step)
CONFIGS = {"nocoef_wd0_step1": (None, 0.0, 1), "coef_wd_step1000": (0.37, 1e-2, 1000)}
GUARD = 8          # poisoned elements in front of every parameter (16 bytes: the parameter itself stays 16-byte aligned unless shifted)
shares = []        # share of p's f32 allowance used, per launch (printed; adam8_ref.P_SHARE_MEASURED records the largest)


@pytest.fixture(scope="module")
def ops():
    from x2i_amd import ops as o
    return o


@pytest.fixture(scope="module")
def qmaps():
    from x2i_amd import optim
    ms, mu = optim.dynamic_map(True).to(DEV), optim.dynamic_map(False).to(DEV)
    return ms, mu, ms.double(), mu.double()


def _loguniform(shape, lo, hi, gen):
    return torch.pow(10.0, lo + (hi - lo) * torch.rand(shape, device=DEV, generator=gen, dtype=torch.float64))


def _kinds(nb):
    """kind of every block [nb]: 0 general (one scale per block, +-1 decade inside), 1 all zero, 2 a single nonzero element, 3 spans 10^4 in |g|
    with no second moment yet, 4 values on map entries and midpoints, 5 the whole range 1e-12 .. 1e4 in one block; sets of fewer than six
    blocks: general"""
    k = torch.arange(nb, device=DEV) % 6
    return k if nb >= 6 else torch.zeros_like(k)


def _gradients(nb, valid, gen, ms64, mu64):
    """f32 [nb, 256]: nonzero |g| within [1e-12, 1e4] (no f32 subnormal in g, g^2 (1 - b2) or the moments), 0 behind a ragged end"""
    kinds = _kinds(nb)
    sign = torch.where(torch.rand((nb, 256), device=DEV, generator=gen) < 0.5, -1.0, 1.0).double()
    g = _loguniform((nb, 1), -11, 3, gen) * _loguniform((nb, 256), -1, 1, gen)
    col = torch.arange(256, device=DEV)
    b2 = torch.nonzero(kinds == 2).view(-1)
    if b2.numel():
        pos = (37 * b2) % valid.sum(1)[b2]
        g[b2] = torch.where(col[None, :] == pos[:, None], _loguniform((b2.numel(), 1), -3, 1, gen), torch.zeros((), device=DEV, dtype=torch.float64))
    b3 = torch.nonzero(kinds == 3).view(-1)
    if b3.numel():
        g3 = _loguniform((b3.numel(), 256), -2, 2, gen)
        g3[:, 0], g3[:, 1] = 100.0, 0.01
        g[b3] = g3
    b4 = torch.nonzero(kinds == 4).view(-1)
    if b4.numel():
        G = 0.125
        i = torch.randint(0, 255, (b4.numel(), 256), device=DEV, generator=gen)
        on_mid = (col % 2 == 1).double()[None, :]
        s = (ms64[i] + on_mid * (ms64[i + 1] - ms64[i]) / 2) * G                 # first moment: m = (1 - b1) g from a zero state
        u = torch.sqrt(mu64[i] + on_mid * (mu64[i + 1] - mu64[i]) / 2) * G       # second moment: v = (1 - b2) g^2
        g4 = torch.where(col[None, :] < 128, s, u)
        g4[:, 0] = G                                                             # the block's largest: x = +-1
        g[b4] = g4
    b5 = torch.nonzero(kinds == 5).view(-1)
    if b5.numel():
        g[b5] = _loguniform((b5.numel(), 256), -12, 4, gen)
    g[kinds == 1] = 0
    return torch.where(valid, (g * sign).float(), torch.zeros((), device=DEV))


class Launch:
    """Parameters (each inside its own poisoned buffer), flat gradients and 8-bit state for one table; run() launches once and checks."""

    def __init__(self, sizes, state, seed, qmaps, misaligned=None):
        self.ms, self.mu, self.ms64, self.mu64 = qmaps
        self.sizes, self.gen = sizes, torch.Generator(device=DEV).manual_seed(seed)
        gen = self.gen
        self.bufs, self.params, self.offs = [], [], []
        for i, n in enumerate(sizes):
            off = GUARD + (3 if i == misaligned else 0)
            buf = poison_(torch.empty(n + 2 * GUARD + 8, device=DEV, dtype=torch.bfloat16))
            p = buf[off:off + n]
            p.copy_((_loguniform((n,), -4, 0, gen) * torch.where(torch.rand(n, device=DEV, generator=gen) < 0.5, -1.0, 1.0)).to(torch.bfloat16))
            self.bufs.append(buf), self.params.append(p), self.offs.append(off)
        _, self.valid = R.to_blocks(self.params)
        nb = self.nb = self.valid.shape[0]
        self.where = [("p%d[%d]" % (i, n), e // 256) for i, n in enumerate(sizes) for e in range(0, n, 256)]
        self.table = torch.tensor([(p.data_ptr() + 2 * e, c) for p, n in zip(self.params, sizes) for _, e, c in R.table_rows_of([n])],
                                  dtype=torch.int64, device=DEV)
        assert self.table.shape == (nb, 2)
        # state: one spare block of codes and eight spare absmax behind the launch's, all poisoned (0x7F bytes / the f32 sentinel)
        self.cm = torch.full(((nb + 1) * 256,), 0x7F, device=DEV, dtype=torch.uint8)
        self.cv = torch.full_like(self.cm, 0x7F)
        self.am = poison_(torch.empty(nb + 8, device=DEV, dtype=torch.float32))
        self.av = poison_(torch.empty(nb + 8, device=DEV, dtype=torch.float32))
        vf = self.valid.view(-1)
        if state == "zero":
            self.cm[:nb * 256][vf] = R.ZERO_SIGNED
            self.cv[:nb * 256][vf] = R.ZERO_UNSIGNED
            self.am[:nb] = 0
            self.av[:nb] = 0
        else:
            self.cm[:nb * 256][vf] = torch.randint(0, 256, (int(vf.sum()),), device=DEV, generator=gen, dtype=torch.uint8)
            self.cv[:nb * 256][vf] = torch.randint(0, 256, (int(vf.sum()),), device=DEV, generator=gen, dtype=torch.uint8)
            self.am[:nb] = _loguniform((nb,), -8, 2, gen).float()
            self.av[:nb] = _loguniform((nb,), -16, 4, gen).float()
            fresh = (_kinds(nb) == 1) | (_kinds(nb) == 3)   # these blocks come with no moments yet: absmax 0 decodes to 0 whatever the codes hold
            self.am[:nb][fresh] = 0
            self.av[:nb][fresh] = 0

    def run(self, ops, name, coef, wd, step):
        nb, vf = self.nb, self.valid.view(-1)
        g = _gradients(nb, self.valid, self.gen, self.ms64, self.mu64)
        before = dict(cm=self.cm[:nb * 256].view(nb, 256).clone(), cv=self.cv[:nb * 256].view(nb, 256).clone(), am=self.am[:nb].clone(),
                      av=self.av[:nb].clone(), p=R.to_blocks(self.params)[0])
        coef_t = None if coef is None else torch.tensor([coef, 12.5], device=DEV, dtype=torch.float32)
        g_flat, table0 = g.view(-1).clone(), self.table.clone()
        ops.adamw8_(self.table, g_flat, self.cm[:nb * 256], self.cv[:nb * 256], self.am[:nb], self.av[:nb], self.ms, self.mu, weight_decay=wd,
                    step=step, coef=coef_t, **HYP)
        torch.cuda.synchronize()
        sc = R.scalars(weight_decay=wd, step=step, **HYP)
        exp = R.expect(before["cm"], before["cv"], before["am"], before["av"], before["p"], g, self.valid,
                       None if coef is None else float(coef_t[0]), sc, self.ms64, self.mu64)
        got_cm, got_cv = self.cm[:nb * 256].view(nb, 256), self.cv[:nb * 256].view(nb, 256)
        share = R.check_step(name, exp, R.to_blocks(self.params)[0], got_cm, got_cv, self.am[:nb], self.av[:nb], self.ms64, self.mu64, self.where)
        shares.append(share)
        print(f"  {name}: {nb} blocks, share of p's f32 allowance used {share:.3f}")
        # what the launch must not write: parameter buffers outside the tensors, codes behind a ragged end and in the spare block, spare absmax,
        # its inputs
        for i, (buf, n, off) in enumerate(zip(self.bufs, self.sizes, self.offs)):
            check_untouched(f"{name}: buffer of parameter {i}", buf, write_mask(buf, [((n,), (1,), off)]))
        for what, c in (("code_m", self.cm), ("code_v", self.cv)):
            keep = (c == 0x7F)
            keep[:nb * 256] |= vf
            assert bool(keep.all()), f"{name}: {what} written behind a block's valid count: first at flat index {int(torch.nonzero(~keep)[0])}"
        assert bool(sentinel_bits(self.am[nb:]).all()) and bool(sentinel_bits(self.av[nb:]).all()), f"{name}: absmax written beyond the last block"
        assert torch.equal(g_flat, g.view(-1)) and torch.equal(self.table, table0), f"{name}: the launch wrote its gradients or its table"
        # the block kinds' own statements
        kinds, v, p_after = _kinds(nb), self.valid, R.to_blocks(self.params)[0]
        k1 = kinds == 1
        m1 = v & k1[:, None]
        assert not bool(self.am[:nb][k1].any()) and not bool(self.av[:nb][k1].any()), f"{name}: absmax of an all-zero block with no moments"
        assert bool((got_cm[m1] == R.ZERO_SIGNED).all()) and bool((got_cv[m1] == R.ZERO_UNSIGNED).all()), f"{name}: codes of such a block"
        decayed = (before["p"].double() * sc["decay"]).float().to(torch.bfloat16)
        assert torch.equal(p_after[m1], decayed[m1]), f"{name}: a block with all-zero gradients and no moments must only decay"
        k3 = kinds == 3
        if bool(k3.any()):
            low = torch.where(v, got_cv, torch.full_like(got_cv, 255)).amin(1)[k3]
            assert bool((low == 1).all()), f"{name}: the small v of a block spanning 10^4 in |g| must take the smallest positive code, never 0"
        k2 = (kinds == 2) & (before["am"] == 0) & (before["av"] == 0)
        assert bool((((got_cm != R.ZERO_SIGNED) & v).sum(1)[k2] == 1).all()) and bool((((got_cv != R.ZERO_UNSIGNED) & v).sum(1)[k2] == 1).all()), \
            f"{name}: a block with one nonzero gradient and no moments holds one nonzero code"
        return exp


@pytest.mark.parametrize("state", ["zero", "random"])
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("pset", list(SETS))
def test_kernel_against_the_float64_checker(ops, qmaps, pset, config, state):
    coef, wd, step = CONFIGS[config]
    L = Launch(SETS[pset], state, 100 + len(pset) + 7 * step, qmaps, misaligned=1 if pset == "three" else None)
    L.run(ops, f"adamw8 {pset} {config} {state}", coef, wd, step)


def test_kernel_grid_stride_reaches_the_blocks_beyond_the_grid(ops, qmaps):
    L = Launch([GRID_STRIDE_N], "random", 7, qmaps)
    assert L.nb == 8192 + 4 > 2048 * 4
    L.run(ops, "adamw8 grid-stride", 0.37, 1e-2, 1000)


def test_three_consecutive_steps_each_from_the_state_the_kernel_left(ops, qmaps):
    L = Launch(SETS["three"], "zero", 21, qmaps, misaligned=1)
    for i in range(3):
        L.run(ops, f"adamw8 three, step {1 + i} of a run", 0.37, 1e-2, 1 + i)
    print(f"  largest share of p's f32 allowance over the launches so far: {max(shares):.3f}")


def test_entry_point_refuses_bad_arguments(ops, qmaps):
    from x2i_amd._lib import X2IError
    L = Launch([512], "zero", 3, qmaps)
    g = torch.zeros(2 * 256 + 4, device=DEV)
    kw = dict(weight_decay=0.0, step=1, **HYP)
    with pytest.raises(X2IError, match="code -1"):
        ops.adamw8_(L.table[:0], g, L.cm, L.cv, L.am, L.av, L.ms, L.mu, **kw)             # no blocks
    with pytest.raises(X2IError, match="code -1"):
        ops.adamw8_(L.table, g[1:], L.cm, L.cv, L.am, L.av, L.ms, L.mu, **kw)             # gradients not 16-byte aligned
    with pytest.raises(X2IError, match="code -1"):
        ops.adamw8_(L.table, g, L.cm[1:], L.cv, L.am, L.av, L.ms, L.mu, **kw)             # codes not 4-byte aligned
    with pytest.raises(X2IError, match="code -1"):
        ops.adamw8_(L.table, g, L.cm, L.cv, L.am, L.av, None, L.mu, **kw)                 # null map


# ------------------------------------------------------------------------------------------------------------------ FlatAdamW8bit.step
MIXED = (("bias", 100), ("w_a", 4096), ("norm", 2048), ("w_ragged", 4352 + 5), ("w_b", 8192))


def _mixed_params(seed):
    gen = torch.Generator().manual_seed(seed)
    return [(n, (0.05 * torch.randn(s, generator=gen)).to(torch.bfloat16).to(DEV)) for n, s in MIXED]


def _exact_sum_grads(n, seed):
    """k / 64, k = -15 .. 15: every partial sum of the squares is an integer multiple of 2^-12 below 2^24 of them, exact in f32 in ANY order --
    the norm, hence the clip coefficient, is then bit-identical whatever the layout of the flat buffer"""
    return torch.randint(-15, 16, (n,), generator=torch.Generator().manual_seed(seed)).float().to(DEV) / 64


def test_flat_adamw8bit_step_against_the_checker_and_flat_adamw(ops, qmaps, monkeypatch):
    from x2i_amd import optim
    ms, mu, ms64, mu64 = qmaps

    class Counted(optim.FlatAdamW8bit):
        hook_calls = 0

        def _weights_changed(self):
            self.hook_calls += 1

    hp = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=1.0)
    opt = Counted(_mixed_params(4), **hp)
    twin = optim.FlatAdamW(_mixed_params(4), **hp)
    large = [n for n, s in MIXED if s >= 4096]
    small = [n for n, s in MIXED if s < 4096]
    assert [opt.names[i] for i in opt.large] == large and opt.blocks == 16 + 18 + 32
    n_large, n_small = sum(s for _, s in MIXED if s >= 4096), sum(s for _, s in MIXED if s < 4096)
    table_bytes = opt.table.numel() * 8
    # 2 codes per element + 8 B of absmax per block of 256 = 2.03125 B per element of a whole block; a ragged parameter's last block is held whole
    # (blocks never straddle parameters), which adds at most 2 * 255 code bytes and its own 8 B of absmax
    assert opt.state_bytes() == 2.03125 * 256 * opt.blocks + 8 * n_small + table_bytes
    assert opt.state_bytes() <= 2.03125 * n_large + 8 * n_small + table_bytes + 1 * (2 * 255 + 8)
    assert table_bytes == 16 * opt.blocks
    calls = dict(a8=0, a32=0)
    real8, real32 = ops.adamw8_, ops.adamw_
    seen = {}

    def count8(table, g, cm, cv, am, av, *a, **k):
        calls["a8"] += 1
        seen.update(cm=cm.clone(), cv=cv.clone(), am=am.clone(), av=av.clone(), g=g.clone(), coef=k["coef"])
        return real8(table, g, cm, cv, am, av, *a, **k)

    def count32(*a, **k):
        calls["a32"] += 1
        return real32(*a, **k)

    monkeypatch.setattr(ops, "adamw8_", count8)
    monkeypatch.setattr(ops, "adamw_", count32)
    where = [(n, e // 256) for n, s in MIXED if s >= 4096 for e in range(0, s, 256)]
    for step in (1, 2):
        for j, (n, s) in enumerate(MIXED):
            gr = _exact_sum_grads(s, 10 * step + j)
            opt.g(n).copy_(gr)
            twin.g(n).copy_(gr)
        p_before = R.to_blocks([opt.params[i] for i in opt.large])[0]
        calls.update(a8=0, a32=0)
        coef = opt.step()
        assert calls == dict(a8=1, a32=len(small)), "ONE 8-bit launch for all large parameters, one f32 launch per small parameter"
        calls.update(a32=0)
        coef_t = twin.step()
        torch.cuda.synchronize()
        assert torch.equal(coef, coef_t) and opt.last_norm is coef and 0.0 < float(coef[0]) < 1.0      # (the clip is active)
        assert opt.hook_calls == step and opt.step_count == step
        assert not bool(opt.grad.any()), "gradients (and the block padding) are zero after the step"
        nb = opt.blocks
        valid = R.to_blocks([opt.params[i] for i in opt.large])[1]
        sc = R.scalars(lr=hp["lr"], beta1=0.9, beta2=0.999, eps=hp["eps"], weight_decay=hp["weight_decay"], step=step)
        exp = R.expect(seen["cm"].view(nb, 256), seen["cv"].view(nb, 256), seen["am"], seen["av"], p_before, seen["g"][:nb * 256].view(nb, 256),
                       valid, float(seen["coef"][0]), sc, ms64, mu64)
        share = R.check_step(f"FlatAdamW8bit.step {step}", exp, R.to_blocks([opt.params[i] for i in opt.large])[0], opt.code_m.view(nb, 256),
                             opt.code_v.view(nb, 256), opt.absmax_m, opt.absmax_v, ms64, mu64, where)
        shares.append(share)
        for n in small:
            i, (o, s) = opt.names.index(n), opt.off[n]
            ot, _ = twin.off[n]
            assert torch.equal(opt.params[i], twin.params[i]), f"small parameter {n} differs from FlatAdamW's"
            assert torch.equal(opt.m[o - opt.small_base:o - opt.small_base + s], twin.m[ot:ot + s])
            assert torch.equal(opt.v[o - opt.small_base:o - opt.small_base + s], twin.v[ot:ot + s])


# ------------------------------------------------------------------------------------------------------------------ trainers
def _tiny_flux():
    """the tiny transformer of tests/test_train_gpu.py / train_distill --tiny"""
    from x2i_amd.flux import FluxTransformer2DModel
    return FluxTransformer2DModel(num_layers=2, num_single_layers=2, num_attention_heads=2, joint_attention_dim=64, pooled_projection_dim=32,
                                  guidance_embeds=True, device=DEV).init_random_(seed=1)


def _tiny_proj(seed=2):
    from x2i_amd.proj import Proj7Exp
    return Proj7Exp(in_channels=5, input_dim=128, output_dim0=32, output_dim1=64, use_t5=False, use_scale=False, use_cnn=True,
                    device=DEV).init_random_(seed)


def _tiny_nets(n, seed=11, out_channels=320):
    """the tiny control nets of tests/test_controlnext_train_gpu.py"""
    from oracle import flux as OF
    from x2i_amd.lightcontrol import ControlNeXtModel
    nets = []
    for i in range(n):
        sd = OF.random_controlnext_state_dict(seed=seed + i, out_channels=out_channels)
        m = ControlNeXtModel(device=DEV, control_out_channels=out_channels)
        m.load_state_dict({k: v.to(torch.bfloat16) for k, v in sd.items()}, strict=True)
        m.compose = False
        nets.append(m)
    return nets


def test_projector_trainer_8bit_lowers_the_loss_and_stays_near_its_f32_twin():
    """Four seeded batches, five passes (20 steps) through both trainers from identical weights.  drift = ||p8 - p32|| / ||p32 - p0|| over all
    parameters: printed (DESIGN.md section 4 records it); the 0.5 is a cap against a run that went somewhere else, not a tolerance (the
    float64 toy of tests/test_adam8_ref_cpu.py gives 0.05 - 0.13 of the parameter norm)."""
    from x2i_amd import optim
    from x2i_amd import train_distill as TD
    from x2i_amd.pipeline import FluxPipeline
    from x2i_amd.train import DistillBackward, ProjectorTrainer, distill_step
    model = _tiny_flux()
    St, lat_hw, bsz = 24, 8, 2
    gen = torch.Generator(device=DEV).manual_seed(5)
    batches = [TD.synthetic_batch(bsz, DEV, gen, model.config, model.inner_dim, St, lat_hw, (5, 128)) for _ in range(4)]
    txt_ids = torch.zeros((St, 3), device=DEV)
    img_ids = FluxPipeline._prepare_latent_image_ids(1, lat_hw, lat_hw, DEV, torch.float32)
    guidance = torch.full((bsz,), 3.5, device=DEV)
    runs = {}
    for eight in (True, False):
        pr = _tiny_proj()
        p0 = torch.cat([p.detach().float().view(-1) for p in pr.parameters()])
        tr = ProjectorTrainer(pr, lr=2e-3, use_8bit_adam=eight)
        assert isinstance(tr, optim.FlatAdamW8bit) == eight
        chain = DistillBackward(model)
        losses = []
        for i in range(20):
            b = batches[i % 4]
            teacher = [b["KD_teacher_tensor0"], b["KD_teacher_tensor1"], b["KD_teacher_tensor2"]]
            losses.append(float(distill_step(tr, chain, b["text_embeddings"], b["latents"], b["timestep"] / 1000, teacher, txt_ids, img_ids,
                                             guidance=guidance)))
        runs[eight] = (losses, torch.cat([p.detach().float().view(-1) for p in pr.parameters()]), p0, tr)
    l8, p8, p0, tr8 = runs[True]
    l32, p32, _, _ = runs[False]
    assert tr8.blocks > 0 and bool(tr8.absmax_v.any()), "the tiny projector has parameters of 4096 elements and more: 8-bit state in use"
    first, last = sum(l8[:4]) / 4, sum(l8[-4:]) / 4
    drift = float((p8 - p32).norm() / (p32 - p0).norm())
    print(f"  8-bit: mean loss of the first pass {first:.4f}, of the last pass {last:.4f} (f32 twin {sum(l32[:4]) / 4:.4f} -> {sum(l32[-4:]) / 4:.4f}); "
          f"drift ||p8 - p32|| / ||p32 - p0|| = {drift:.4f}")
    assert all(math.isfinite(v) for v in l8) and last < first
    assert drift <= 0.5


def test_controlnext_trainer_8bit_step_updates_and_drops_caches():
    from x2i_amd import optim
    from x2i_amd.lightcontrol_train import ControlNeXtTrainer
    nets = _tiny_nets(2)
    # (lr 1e-2: a first Adam step moves every element by lr, which must exceed half a bf16 ulp of weights near 1 for each tensor to change)
    tr = ControlNeXtTrainer(nets, lr=1e-2, max_grad_norm=0.5, use_8bit_adam=True)
    assert isinstance(tr, optim.FlatAdamW8bit) and isinstance(tr, ControlNeXtTrainer) and tr.blocks > 0 and len(tr.small) > 0
    hint = (torch.rand((1, 3, 128, 128), generator=torch.Generator().manual_seed(12)) * 2 - 1).to(torch.bfloat16).float().to(DEV)
    t = torch.tensor([500.0], device=DEV)
    before = [n(hint, t)["out"].clone() for n in nets]        # fills the packed-weight caches
    tr.forward(hint, t)
    assert tr.saved is not None
    old = [p.detach().clone() for p in tr.params]
    for j, n in enumerate(tr.names):
        tr.g(n).copy_(1e-2 * torch.randn(tr.g(n).numel(), generator=torch.Generator().manual_seed(100 + j)).to(DEV))
    coef = tr.step()
    assert 0.0 < float(coef[0]) < 1.0 and tr.saved is None and not bool(tr.grad.any())
    for n, p, q in zip(tr.names, tr.params, old):
        assert bool(torch.isfinite(p.float()).all()), n
        assert not torch.equal(p, q), f"{n} did not change"
    for net, b0 in zip(nets, before):
        after = net(hint, t)["out"]
        assert not torch.equal(after, b0)
        fresh = type(net)(device=DEV, control_out_channels=320)
        fresh.load_state_dict(net.state_dict())
        fresh.compose = False
        assert torch.equal(after, fresh(hint, t)["out"]), "a weight-derived cache survived the 8-bit step"


def test_training_program_with_the_flag(tmp_path):
    from x2i_amd import optim
    from x2i_amd import train_distill as TD
    losses = TD.main(["--synthetic", "--tiny", "--use_8bit_adam", "--max_train_steps", "6", "--batch_size", "2", "--learning_rate", "1e-3",
                      "--checkpointing_steps", "1000", "--output_dir", str(tmp_path), "--seed", "1"])
    assert len(losses) == 6 and all(math.isfinite(v) for v in losses)
    tr = TD.run.last["trainer"]
    assert isinstance(tr, optim.FlatAdamW8bit) and tr.step_count == 6 and tr.code_m.dtype == torch.uint8
    assert bool(tr.absmax_m.any()) and bool(tr.absmax_v.any()) and bool((tr.code_v != 0).any())


def test_default_trainers_are_bit_identical_to_a_direct_flat_adamw_run():
    """use_8bit_adam left at its default: the same class, the same launches, the same bits as FlatAdamW on the same gradients.  (Uses nothing
    this change added: it passes on both sides of it.)"""
    from x2i_amd.lightcontrol_train import ControlNeXtTrainer
    from x2i_amd.optim import FlatAdamW
    from x2i_amd.train import ProjectorTrainer
    hp = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=0.5)

    def compare(tr, direct):
        assert tr.names == direct.names and tr.off == direct.off
        for step in (1, 2):
            gr = 1e-2 * torch.randn(tr.grad.numel(), generator=torch.Generator().manual_seed(step)).to(DEV)
            tr.grad.copy_(gr)
            direct.grad.copy_(gr)
            a, b = tr.step(), direct.step()
            assert torch.equal(a, b)
            assert torch.equal(tr.m, direct.m) and torch.equal(tr.v, direct.v)
            for n, p, q in zip(tr.names, tr.params, direct.params):
                assert torch.equal(p, q), n

    pr = _tiny_proj()
    tr = ProjectorTrainer(pr, **hp)
    assert type(tr) is ProjectorTrainer and isinstance(tr, FlatAdamW)
    compare(tr, FlatAdamW(_tiny_proj().named_parameters(), **hp))
    nets = _tiny_nets(1)
    tr = ControlNeXtTrainer(nets, **hp)
    assert type(tr) is ControlNeXtTrainer and isinstance(tr, FlatAdamW)
    compare(tr, FlatAdamW((("0." + n, p) for n, p in _tiny_nets(1)[0].named_parameters()), **hp))
