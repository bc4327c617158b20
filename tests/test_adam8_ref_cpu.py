"""The float64 reference of the block-wise 8-bit AdamW step (tests/adam8_ref.py) and its checker, on the CPU: the code maps have the stated
properties, the checker accepts the reference's own output and rejects the mistakes a kernel of this kind makes, the float64 statement of the
format stays close to plain AdamW on the toy problem -- and does not without the positive-v rule -- and the training program has the flag."""
import numpy as np
import pytest
import torch

from tests import adam8_ref as R
from tests.gemm_ref import bf16_rne

SC = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2)


def test_dynamic_maps_have_the_stated_properties():
    from x2i_amd import optim
    for signed, lowest, smallest_pos, zero_at in ((True, -0.99296875, 5.5e-7, 127), (False, 0.0, 3.25e-7, 0)):
        m = optim.dynamic_map(signed)
        assert m.dtype == torch.float32 and m.shape == (256,)
        assert bool((m[1:] > m[:-1]).all()), "strictly increasing"
        assert int((m == 0).sum()) == 1 and int((m == 0).nonzero()[0]) == zero_at
        assert float(m.max()) == 1.0 and float(m.min()) == float(np.float32(lowest))
        assert float(m[m > 0].min()) == float(np.float32(smallest_pos))
        assert int((m < 0).sum()) == (127 if signed else 0)
        assert np.array_equal(m.numpy(), R.dynamic_map_f64(signed).astype(np.float32)), "the package's map is the format's definition rounded to f32"
    assert (R.ZERO_SIGNED, R.ZERO_UNSIGNED) == (127, 0)


@pytest.fixture(scope="module")
def case():
    """Three blocks of one parameter of 2 * 256 + 100 elements (the last ragged) after one reference step from random incoming state; the
    padding of the ragged block holds large gradients and random codes, as a kernel reading it would find."""
    gen = torch.Generator().manual_seed(5)
    ms, mu = R.maps()
    B = 3
    valid = torch.ones((B, 256), dtype=torch.bool)
    valid[2, 100:] = False
    cm = torch.randint(0, 256, (B, 256), generator=gen)
    cv = torch.randint(0, 256, (B, 256), generator=gen)
    am = (torch.rand(B, generator=gen) * 0.1 + 0.01).float()
    av = (torch.rand(B, generator=gen) * 1e-3 + 1e-4).float()
    p = (torch.randn((B, 256), generator=gen) * 0.01).to(torch.bfloat16)
    g = (torch.randn((B, 256), generator=gen) * torch.logspace(-2, 0, 256)[torch.randperm(256, generator=gen)]).float()
    cv[1, :64] = 0               # block 1: elements without a second moment yet and gradients 10^4 below the block's largest
    g[1, :64] = 1e-4 * torch.sign(g[1, :64]) * (0.5 + torch.rand(64, generator=gen))
    g_pad = g.clone()
    g_pad[2, 100:] = 50.0        # what sits behind the ragged end
    sc = R.scalars(step=7, **SC)
    exp = R.expect(cm, cv, am, av, p, g_pad, valid, 0.5, sc, ms, mu)
    got = dict(p=bf16_rne(exp["p"]).to(torch.bfloat16), am=exp["am"].float(),
               av=exp["av"].float(), cm=R.quantise(exp["xm"], ms), cv=R.quantise(exp["xv"], mu, True))
    return dict(exp=exp, got=got, ms=ms, mu=mu, sc=sc, state=(cm, cv, am, av, p, g_pad, valid), where=[("w", b) for b in range(B)])


def _check(c, **repl):
    g = dict(c["got"], **repl)
    return R.check_step("case", c["exp"], g["p"], g["cm"], g["cv"], g["am"], g["av"], c["ms"], c["mu"], c["where"])


def test_checker_accepts_the_reference_rounded_to_f32(case):
    share = _check(case)
    assert share <= 1.0


def test_checker_rejects_a_code_off_by_one_away_from_a_midpoint(case):
    ms, exp = case["ms"], case["exp"]
    mid = (ms[1:] + ms[:-1]) / 2
    k = case["got"]["cm"]
    # an element whose value is at least a thousand bounds away from both ends of its cell, with neighbours on both sides
    d_lo = exp["xm"] - mid[(k - 1).clamp(0, 254)]
    d_hi = mid[k.clamp(0, 254)] - exp["xm"]
    far = exp["valid"] & (k > 0) & (k < 255) & (d_lo > 1e3 * exp["dxm"]) & (d_hi > 1e3 * exp["dxm"])
    b, e = (int(i) for i in torch.nonzero(far)[0])
    for off in (1, -1):
        bad = k.clone()
        bad[b, e] += off
        with pytest.raises(AssertionError, match=rf"code_m of 1 elements.*parameter w, block {b} .*element {e} "):
            _check(case, cm=bad)


def test_checker_rejects_an_absmax_over_the_padding_of_a_ragged_block(case):
    cm, cv, am, av, p, g, valid = case["state"]
    full = R.expect(cm, cv, am, av, p, g, torch.ones_like(valid), 0.5, case["sc"], case["ms"], case["mu"])
    assert float(full["am"][2]) > float(case["exp"]["am"][2])
    with pytest.raises(AssertionError, match=r"absmax_m of 1 blocks.*parameter w, block 2"):
        _check(case, am=full["am"].float())
    with pytest.raises(AssertionError, match=r"absmax_v of 1 blocks.*parameter w, block 2"):
        _check(case, av=full["av"].float())


def test_checker_rejects_a_zero_code_for_a_positive_v(case):
    exp = case["exp"]
    # where plain nearest rounding gives 0 although v > 0 (the deviation from bitsandbytes), and anywhere else
    plain = R.quantise(exp["xv"], case["mu"])
    small = exp["valid"] & (exp["v"] > 0) & (plain == 0)
    assert bool(small.any()), "the case has second moments below half the smallest positive entry"
    with pytest.raises(AssertionError, match=r"code_v of \d+ elements.*zero index is never accepted"):
        _check(case, cv=plain)
    assert bool((case["got"]["cv"][small] == 1).all())
    bad = case["got"]["cv"].clone()
    bad[0, 3] = 0
    with pytest.raises(AssertionError, match=r"code_v of 1 elements.*block 0 .*element 3 "):
        _check(case, cv=bad)


def test_checker_rejects_p_from_the_quantised_moments(case):
    exp, sc, g = case["exp"], case["sc"], case["got"]
    mq = case["ms"][g["cm"]] * exp["am"][:, None]
    vq = case["mu"][g["cv"]] * exp["av"][:, None]
    p_old = case["state"][4].double()
    pq = p_old * sc["decay"] - sc["lr"] * (mq / sc["bc1"]) / ((vq / sc["bc2"]).sqrt() + sc["eps"])
    with pytest.raises(AssertionError, match=r"p of \d+ elements over the bound"):
        _check(case, p=pq.float().to(torch.bfloat16))


def test_checker_rejects_a_blocks_state_written_into_its_neighbour(case):
    g = case["got"]
    roll = lambda t: torch.roll(t, 1, 0)  # noqa: E731
    with pytest.raises(AssertionError, match=r"absmax_m of \d blocks.*code_m of \d+ elements"):
        _check(case, cm=roll(g["cm"]), cv=roll(g["cv"]), am=roll(g["am"]), av=roll(g["av"]))
    with pytest.raises(AssertionError, match=r"code_m of \d+ elements"):
        _check(case, cm=roll(g["cm"]))


def test_float64_format_stays_close_to_adamw_on_the_toy_and_needs_the_positive_v_rule():
    """seed 0, n = 4096, gradient scales logspace(-1.5, 1.5) permuted (every block spans 1000x), lr 1e-3, wd 1e-2, 200 steps.  Measured when
    the format was decided: 0.119 with the rule, 4.16 without (the loss rises).  The bound is twice the former: a tie rule may differ."""
    with_rule = R.toy_distance(True)
    without = R.toy_distance(False)
    print(f"toy: ||p8 - p32|| / ||p32|| = {with_rule:.4f} with the positive-v rule, {without:.4f} without")
    assert with_rule <= 0.25
    assert without > 1.0


def test_train_distill_has_the_flag():
    from x2i_amd import train_distill
    assert train_distill.parse_args([]).use_8bit_adam is False
    assert train_distill.parse_args(["--use_8bit_adam"]).use_8bit_adam is True


def test_8bit_optimizer_bookkeeping_on_the_cpu_device():
    """FlatAdamW8bit built without a launch: large parameters first, each on a block boundary, small ones behind; one table row per block."""
    from x2i_amd import optim
    sizes = dict(a=100, w0=4096, b=7, w1=4352 + 5, w2=8192)
    params = [(n, torch.zeros(s, dtype=torch.bfloat16)) for n, s in sizes.items()]
    opt = optim.FlatAdamW8bit(params, 1e-3, (0.9, 0.999), 1e-8, 1e-2, 1.0)
    assert opt.names == list(sizes) and list(opt.named_grads()) == list(sizes)
    assert opt.off["w0"] == (0, 4096) and opt.off["w1"] == (4096, 4357) and opt.off["w2"] == (4096 + 18 * 256, 8192)
    assert opt.blocks == 16 + 18 + 32 and opt.off["a"] == (opt.blocks * 256, 100) and opt.off["b"] == (opt.blocks * 256 + 100, 7)
    assert opt.grad.numel() == opt.blocks * 256 + 107 and opt.m.numel() == opt.v.numel() == 107
    rows = opt.table.tolist()
    want = [(p.data_ptr() + 2 * e, c) for i, e, c in R.table_rows_of([4096, 4357, 8192]) for p in [params[[1, 3, 4][i]][1]]]
    assert [tuple(r) for r in rows] == want and rows[16 + 17][1] == 5
    assert opt.state_bytes() == opt.blocks * (2 * 256 + 8 + 16) + 8 * 107
    assert bool((opt.absmax_m == 0).all()) and opt.code_m.dtype == torch.uint8 and opt.code_m.numel() == opt.blocks * 256
    # the trainers: the default is the class itself, the option its 8-bit variant
    from x2i_amd.proj import Proj7Exp
    from x2i_amd.train import ProjectorTrainer
    pr = Proj7Exp(in_channels=3, input_dim=16, output_dim0=8, output_dim1=24, use_t5=False, use_scale=False, use_cnn=True, device="cpu")
    assert type(ProjectorTrainer(pr)) is ProjectorTrainer and not isinstance(ProjectorTrainer(pr), optim.FlatAdamW8bit)
    t8 = ProjectorTrainer(pr, use_8bit_adam=True)
    assert isinstance(t8, ProjectorTrainer) and isinstance(t8, optim.FlatAdamW8bit) and t8.proj is pr
