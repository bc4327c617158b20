"""ControlNeXt backward on the HIP path (x2i_amd/lightcontrol_train.py, csrc/conv_bwd.hip): the weight-gradient, stem, GroupNorm-backward and
data-gradient launches against float64 on the same bf16 operands, the whole net's gradients against autograd through oracle.flux.controlnext_forward,
and ControlNeXtTrainer's optimizer step, cache invalidation and checkpoint round trip."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import flux as OF
from tests.cnx_bwd_ref import _wgrad_bound_terms
from tests.util import seeded

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24


def bf(x):
    return x.to(torch.bfloat16)


def rb(x):
    return x.to(torch.bfloat16).float()


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


# -------------------------------------------------------------------------------------------------------------- conv weight gradient
# (Cin, Cout, k, stride, pad, B, H, W): the table's layers on reduced grids, B = 1 / 2 / 3 and a non-square grid
WGRAD_CASES = [(64, 64, 3, 1, 1, 2, 48, 48), (64, 128, 3, 1, 1, 1, 40, 56), (128, 128, 3, 1, 1, 3, 32, 32), (128, 128, 3, 2, 1, 2, 64, 48),
               (128, 256, 3, 1, 1, 2, 24, 40), (256, 256, 3, 1, 1, 2, 32, 32), (128, 256, 1, 1, 0, 2, 32, 24), (256, 256, 3, 2, 1, 1, 48, 64),
               (256, 3072, 2, 2, 0, 2, 16, 16)]


@pytest.mark.parametrize("Cin,Cout,k,s,p,B,H,W", WGRAD_CASES)
def test_conv_wgrad_per_element_against_float64(Cin, Cout, k, s, p, B, H, W):
    from x2i_amd import ops
    x = bf(seeded((B, Cin, H, W), 1))
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dy = bf(seeded((B, Cout, OH, OW), 2))
    want = torch.nn.grad.conv2d_weight(x.double(), (Cout, Cin, k, k), dy.double(), stride=s, padding=p)
    absum = torch.nn.grad.conv2d_weight(x.double().abs(), (Cout, Cin, k, k), dy.double().abs(), stride=s, padding=p)
    dbw = dy.double().sum((0, 2, 3))
    dbabs = dy.double().abs().sum((0, 2, 3))
    xg, dyg = _nhwc(x).to(DEV), _nhwc(dy).to(DEV)
    dw = torch.full((Cout, Cin, k, k), float("nan"), device=DEV)
    db = torch.full((Cout,), float("nan"), device=DEV)
    ops.conv_wgrad(xg, dyg, dw, db, H, W, Cin, OH, OW, Cout, k, k, s, p)
    steps, nsplit = _wgrad_bound_terms(B, OH, OW, Cin, Cout, k)
    gam = (32 + steps + nsplit) * U
    err = (dw.double().cpu() - want).abs()
    bound = gam * absum + U * want.abs() + 1e-30
    frac = (err / bound).max().item()
    print("wgrad %s: steps %d splits %d, max err / bound %.4f" % ((Cin, Cout, k, s, B, H, W), steps, nsplit, frac))
    assert frac <= 1.0
    errb = (db.double().cpu() - dbw).abs()
    assert (errb <= gam * dbabs + U * dbw.abs() + 1e-30).all()
    # bit-identical relaunch; accumulate adds into what is there
    dw2, db2 = torch.empty_like(dw), torch.empty_like(db)
    ops.conv_wgrad(xg, dyg, dw2, db2, H, W, Cin, OH, OW, Cout, k, k, s, p)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    ops.conv_wgrad(xg, dyg, dw2, db2, H, W, Cin, OH, OW, Cout, k, k, s, p, accumulate=True)
    assert torch.equal(dw2, dw + dw) and torch.equal(db2, db + db)


def test_conv_wgrad_reads_strided_token_rows():
    """dy given as the image rows of a wider token buffer (offset, row stride, batch stride), the way forward_nhwc's add_into addresses it."""
    from x2i_amd import ops
    B, Cin, Cout, H, W = 2, 256, 384, 16, 12
    x = bf(seeded((B, H, W, Cin), 3)).to(DEV)
    dy = bf(seeded((B, H // 2 * W // 2, Cout), 4)).to(DEV)
    S, St, ld = H // 2 * W // 2 + 5, 5, Cout + 64
    buf = torch.zeros((B, S, ld), device=DEV, dtype=torch.bfloat16)
    buf[:, St:, :Cout] = dy
    a, b = torch.empty((Cout, Cin, 2, 2), device=DEV), torch.empty((Cout,), device=DEV)
    ops.conv_wgrad(x, dy, a, b, H, W, Cin, H // 2, W // 2, Cout, 2, 2, 2, 0)
    c, d = torch.empty_like(a), torch.empty_like(b)
    ops.conv_wgrad(x, buf, c, d, H, W, Cin, H // 2, W // 2, Cout, 2, 2, 2, 0, dy_offset=St * ld, dy_batch_stride=S * ld, ldy=ld)
    assert torch.equal(a, c) and torch.equal(b, d)


def test_conv_stem_wgrad_against_float64():
    from x2i_amd import ops
    B, H, W = 3, 50, 36
    x = bf(seeded((B, 3, H, W), 5))
    dy = bf(seeded((B, 64, H // 2, W // 2), 6))
    want = torch.nn.grad.conv2d_weight(x.double(), (64, 3, 3, 3), dy.double(), stride=2, padding=1)
    absum = torch.nn.grad.conv2d_weight(x.double().abs(), (64, 3, 3, 3), dy.double().abs(), stride=2, padding=1)
    dw, db = torch.empty((64, 3, 3, 3), device=DEV), torch.empty((64,), device=DEV)
    ops.conv_stem_wgrad(_nhwc(x).to(DEV), _nhwc(dy).to(DEV), dw, db)
    P = B * (H // 2) * (W // 2)
    gam = (P / 1024 / 4 + 1024 + 8) * U     # per-thread run of a block, the four threads, then the blocks
    assert ((dw.double().cpu() - want).abs() <= gam * absum + 1e-30).all()
    assert torch.allclose(db.double().cpu(), dy.double().sum((0, 2, 3)), rtol=1e-5, atol=1e-3)


# -------------------------------------------------------------------------------------------------------------- GroupNorm backward
# (C, G, eps, act, pre_add, in_relu): every combination the net runs
GN_CASES = [(64, 2, 1e-5, 4, False, False), (128, 2, 1e-5, 4, False, False), (128, 4, 1e-6, 3, False, False), (128, 4, 1e-6, 3, True, False),
            (128, 8, 1e-6, 3, False, False), (256, 8, 1e-6, 3, True, False), (256, 8, 1e-5, 0, False, False), (256, 8, 1e-5, 0, False, True)]


@pytest.mark.parametrize("C,G,eps,act,pre,in_relu", GN_CASES)
def test_groupnorm_bwd_against_float64_autograd(C, G, eps, act, pre, in_relu):
    from x2i_amd import ops
    B, H, W = 2, 20, 28
    x = bf(seeded((B, C, H, W), 7, 1.5) + 0.3)
    if in_relu:
        x = bf(torch.relu(x.float()))
    w, b = bf(1 + 0.2 * seeded((C,), 8)), bf(0.2 * seeded((C,), 9))
    pa = seeded((B, C), 10) if pre else None
    dy = bf(seeded((B, C, H, W), 11))
    dxin = bf(seeded((B, C, H, W), 12))
    fn = {0: lambda t: t, 3: F.silu, 4: F.relu}[act]
    xd = x.double().requires_grad_()
    wd, bd = w.double().requires_grad_(), b.double().requires_grad_()
    pd = pa.double().requires_grad_() if pre else None
    xin = xd + pd[:, :, None, None] if pre else xd
    y = fn(F.group_norm(xin, G, wd, bd, eps))
    y.backward(dy.double())
    gx = xd.grad * (x.double() > 0) if in_relu else xd.grad
    dx_ref = gx + dxin.double()
    dw, db = torch.zeros((C,), device=DEV), torch.zeros((C,), device=DEV)
    dpre = torch.empty((B, C), device=DEV) if pre else None
    dx = ops.groupnorm_bwd(_nhwc(x).to(DEV), _nhwc(dy).to(DEV), w.to(DEV), b.to(DEV), G, eps, act=act, pre_add=pa.to(DEV) if pre else None, dpre=dpre,
                           dx_in=_nhwc(dxin).to(DEV), dw=dw, db=db, in_relu=in_relu, accumulate=True)
    dx = dx.permute(0, 3, 1, 2).double().cpu()

    def rel(a, r):
        return ((a - r).norm() / r.norm()).item()
    # dx: one bf16 rounding of an f32 evaluation
    assert rel(dx, dx_ref) < 6e-3
    assert rel(dw.double().cpu(), wd.grad) < 1e-4 and rel(db.double().cpu(), bd.grad) < 1e-4
    if pre:
        # d pre_add cancels within each group: bound against the scale of the per-channel sums it is made of
        scale = (gx.abs().sum((2, 3))).max()
        assert ((dpre.double().cpu() - pd.grad).abs() <= 1e-4 * scale).all()
    dx2 = ops.groupnorm_bwd(_nhwc(x).to(DEV), _nhwc(dy).to(DEV), w.to(DEV), b.to(DEV), G, eps, act=act, pre_add=pa.to(DEV) if pre else None,
                            dx_in=_nhwc(dxin).to(DEV), in_relu=in_relu)
    assert torch.equal(dx2.permute(0, 3, 1, 2).double().cpu(), dx)


# -------------------------------------------------------------------------------------------------------------- data gradients
def _rel(a, r):
    return ((a.double() - r).norm() / r.norm()).item()


def test_every_data_gradient_form_against_conv2d_input():
    from x2i_amd import ops
    from x2i_amd import lightcontrol_train as LT
    B = 2
    # 3x3 s1 p1 with a residual gradient
    for ci, co, H, W in [(64, 64, 20, 28), (64, 128, 16, 24), (256, 256, 12, 10)]:
        w = bf(seeded((co, ci, 3, 3), 20) / (9 * ci) ** 0.5)
        dy, res = bf(seeded((B, co, H, W), 21)), bf(seeded((B, ci, H, W), 22))
        want = torch.nn.grad.conv2d_input((B, ci, H, W), w.double(), dy.double(), padding=1) + res.double()
        got = ops.conv2d_nhwc(_nhwc(dy).to(DEV), LT.dgrad_weight_3x3(w.to(DEV)), None, H, W, co, ci, 3, 3, 1, 1, res=_nhwc(res).to(DEV))
        assert _rel(got.permute(0, 3, 1, 2).cpu(), want) < 6e-3
    # 3x3 s2 p1: four interleaved phases
    for c, oh, ow in [(128, 12, 20), (256, 8, 6)]:
        w = bf(seeded((c, c, 3, 3), 23) / (9 * c) ** 0.5)
        dy = bf(seeded((B, c, oh, ow), 24))
        want = torch.nn.grad.conv2d_input((B, c, 2 * oh, 2 * ow), w.double(), dy.double(), stride=2, padding=1)
        got = LT.dgrad_s2(_nhwc(dy).to(DEV), w.to(DEV), oh, ow)
        assert _rel(got.permute(0, 3, 1, 2).cpu(), want) < 6e-3
    # 1x1
    w = bf(seeded((256, 128, 1, 1), 25) / 128 ** 0.5)
    dy = bf(seeded((B, 256, 10, 14), 26))
    want = torch.nn.grad.conv2d_input((B, 128, 10, 14), w.double(), dy.double())
    got = ops.conv2d_nhwc(_nhwc(dy).to(DEV), LT.dgrad_weight_1x1(w.to(DEV)), None, 10, 14, 256, 128, 1, 1, 1, 0)
    assert _rel(got.permute(0, 3, 1, 2).cpu(), want) < 6e-3
    # 2x2 stride 2, dY as strided token rows
    w = bf(seeded((3072, 256, 2, 2), 27) / 1024 ** 0.5)
    ho, wo = 6, 8
    dy = bf(seeded((B, 3072, ho, wo), 28))
    want = torch.nn.grad.conv2d_input((B, 256, 2 * ho, 2 * wo), w.double(), dy.double(), stride=2)
    S, St = ho * wo + 3, 3
    buf = torch.zeros((B, S, 3072), device=DEV, dtype=torch.bfloat16)
    buf[:, St:] = dy.permute(0, 2, 3, 1).reshape(B, ho * wo, 3072).to(DEV)
    got = LT.dgrad_2x2s2(buf, w.to(DEV), B, ho, wo, offset=St * 3072, ld=3072, batch_stride=S * 3072)
    assert _rel(got.permute(0, 3, 1, 2).cpu(), want) < 6e-3


# -------------------------------------------------------------------------------------------------------------- whole net
def _nets(n, seed=0, out_channels=3072):
    from x2i_amd.lightcontrol import ControlNeXtModel
    nets, sds = [], []
    for i in range(n):
        sd = OF.random_controlnext_state_dict(seed=seed + i, out_channels=out_channels)
        m = ControlNeXtModel(device=DEV, control_out_channels=out_channels)
        m.load_state_dict({k: bf(v) for k, v in sd.items()}, strict=True)
        m.compose = False
        nets.append(m)
        sds.append({k: rb(v) for k, v in sd.items()})
    return nets, sds


def _oracle_grads(sd, hint, t, g, dtype):
    p = {k: v.to(dtype).requires_grad_() for k, v in sd.items()}
    out = OF.controlnext_forward(p, "", hint.to(dtype), torch.tensor([t], dtype=torch.float64))["out"]
    (out.double() * g.double()).sum().backward()
    return {k: v.grad.double() for k, v in p.items()}


# conv biases directly in front of a GroupNorm (their gradients cancel within each group), with the conv whose weight gradient sets their scale
CANCELLING = {"embedding.0.bias": "embedding.0.weight", "embedding.3.bias": "embedding.3.weight", "embedding.6.bias": "embedding.6.weight",
              "down_res.0.conv1.bias": "down_res.0.conv1.weight", "down_res.1.conv1.bias": "down_res.1.conv1.weight",
              "mid_convs.0.3.bias": "mid_convs.0.3.weight", "down_res.0.time_emb_proj.bias": "down_res.0.time_emb_proj.weight",
              "down_res.1.time_emb_proj.bias": "down_res.1.time_emb_proj.weight"}


@pytest.mark.parametrize("B,H", [(2, 128), (2, 256), (1, 512)])
def test_trainer_backward_against_float64_autograd(B, H):
    """ControlNeXtTrainer.backward vs autograd through the oracle in float64 on the same bf16 weights and hint, random upstream gradient: per
    parameter at most ~1.5x the error of PyTorch's own bf16 autograd (the reference trains in bf16).  512^2 stands for 1024^2: the float64 CPU
    oracle takes several minutes there."""
    from x2i_amd.lightcontrol_train import ControlNeXtTrainer
    nets, sds = _nets(1, seed=3)
    hint = rb(torch.rand((B, 3, H, H), generator=torch.Generator().manual_seed(4)) * 2 - 1)
    t = 640.0
    tr = ControlNeXtTrainer(nets)
    out = tr.forward(hint.to(DEV), torch.tensor([t], device=DEV))[0]
    ref = nets[0](hint.to(DEV), torch.tensor([t], device=DEV))["out"].permute(0, 2, 3, 1)
    assert torch.equal(out, ref)                             # the same launches as ControlNeXtModel.forward on the chained form
    if (B, H) == (2, 128):                                   # the trainer ignores net.compose: it always trains the chained form
        nets[0].compose = True
        assert torch.equal(tr.forward(hint.to(DEV), torch.tensor([t], device=DEV))[0], ref)
        nets[0].compose = False
    g = bf(seeded(tuple(out.shape), 5))
    tr.backward([g.to(DEV)])
    hip = {k: v.double().cpu() for k, v in tr.named_grads().items()}
    gn = g.permute(0, 3, 1, 2)
    g64 = _oracle_grads(sds[0], hint, t, gn, torch.float64)
    g16 = _oracle_grads(sds[0], hint, t, gn, torch.bfloat16)
    worst, bad = 0.0, []
    for k, ref64 in g64.items():
        e_hip = (hip["0." + k] - ref64).norm().item()
        e_bf = (g16[k] - ref64).norm().item()
        if k in CANCELLING:
            scale = g64[CANCELLING[k]].norm().item() / g64[CANCELLING[k]].numel() ** 0.5 * ref64.numel() ** 0.5
            ok = e_hip <= max(1.5 * e_bf, 2e-2 * scale)
        else:
            ok = e_hip <= max(1.5 * e_bf, 1e-3 * ref64.norm().item())
        worst = max(worst, e_hip / max(e_bf, 1e-30))
        print("%-40s hip %.3e  bf16 %.3e  |g| %.3e" % (k, e_hip, e_bf, ref64.norm().item()))
        if not ok:
            bad.append(k)
    print("worst hip / bf16 error ratio %.3f" % worst)
    assert not bad, bad
    # two runs of the backward are bit-identical
    first = tr.grad.clone()
    tr.zero_grad()
    tr.backward([g.to(DEV)])
    assert torch.equal(first, tr.grad)


# -------------------------------------------------------------------------------------------------------------- optimizer
def test_step_matches_clip_grad_norm_and_torch_adamw_and_invalidates_caches():
    from x2i_amd.lightcontrol import make_control_fn
    from x2i_amd.lightcontrol_train import ControlNeXtTrainer
    nets, sds = _nets(2, seed=11, out_channels=320)
    tr = ControlNeXtTrainer(nets, lr=1e-3, max_grad_norm=0.5)
    hint = rb(torch.rand((1, 3, 128, 128), generator=torch.Generator().manual_seed(12)) * 2 - 1).to(DEV)
    tref = torch.tensor([500.0], device=DEV)
    before = [n(hint, tref)["out"].clone() for n in nets]        # fills the packed-weight caches
    grads = seeded((tr.grad.numel(),), 13, 1e-2).to(DEV)
    tr.grad.copy_(grads)
    params = [p.detach().clone().requires_grad_() for p in tr.params]
    opt = torch.optim.AdamW(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    for p, n in zip(params, tr.names):
        o, s = tr.off[n]
        p.grad = grads[o:o + s].view(p.shape).to(torch.bfloat16)
    torch.nn.utils.clip_grad_norm_(params, 0.5)
    opt.step()
    coef = tr.step()
    assert abs(coef[1].item() - grads.norm().item()) <= 1e-4 * grads.norm().item()
    for p, q in zip(tr.params, params):
        assert (p.float() - q.float()).abs().max().item() <= 2 * (2.0 ** -8) * q.float().abs().max().item() + 1e-6
    # the forward of every path sees the updated weights (the packed caches were dropped)
    for n, b0, sd_i in zip(nets, before, range(2)):
        after = n(hint, tref)["out"]
        assert not torch.equal(after, b0)
        fresh = type(n)(device=DEV, control_out_channels=320)
        fresh.load_state_dict(n.state_dict())
        fresh.compose = False
        assert torch.equal(after, fresh(hint, tref)["out"])
    for n in nets:
        n.compose = True
    X = torch.zeros((1, 64 + 16, 320), device=DEV, dtype=torch.bfloat16)
    fn = make_control_fn(nets, hint)
    fn(0, tref, X, 16, 80, 320)
    fresh = type(nets[0])(device=DEV, control_out_channels=320)
    fresh.load_state_dict(nets[0].state_dict())
    Y = torch.zeros_like(X)
    make_control_fn([fresh], hint)(0, tref, Y, 16, 80, 320)
    assert torch.equal(X, Y)


def test_two_rounds_match_the_oracle_at_the_updated_weights():
    """forward / backward / step twice: the second round's gradients are the oracle's at the weights after the first step (stale packed
    weights would show here)."""
    from x2i_amd.lightcontrol_train import ControlNeXtTrainer
    nets, _ = _nets(1, seed=21, out_channels=320)
    tr = ControlNeXtTrainer(nets, lr=1e-2)
    hint = rb(torch.rand((2, 3, 128, 128), generator=torch.Generator().manual_seed(22)) * 2 - 1)
    g = bf(seeded((2, 8, 8, 320), 23))
    for rnd in range(2):
        tr.forward(hint.to(DEV), torch.tensor([300.0], device=DEV))
        tr.backward([g.to(DEV)])
        hip = {k[2:]: v.double().cpu() for k, v in tr.named_grads().items()}
        sd = {k: v.detach().float().cpu() for k, v in nets[0].state_dict().items()}
        g64 = _oracle_grads(sd, hint, 300.0, g.permute(0, 3, 1, 2), torch.float64)
        g16 = _oracle_grads(sd, hint, 300.0, g.permute(0, 3, 1, 2), torch.bfloat16)
        for k in ("mid_convs.1.weight", "down_res.0.conv2.weight", "embedding.3.weight", "time_embedding.linear_1.weight"):
            e_hip, e_bf = (hip[k] - g64[k]).norm().item(), (g16[k] - g64[k]).norm().item()
            assert e_hip <= max(1.5 * e_bf, 1e-3 * g64[k].norm().item()), (rnd, k, e_hip, e_bf)
        tr.step()


# -------------------------------------------------------------------------------------------------------------- end to end
def test_training_lowers_the_loss_names_and_checkpoint_round_trip(tmp_path):
    from x2i_amd import checkpoints
    from x2i_amd.lightcontrol_train import ControlNeXtTrainer
    nets, _ = _nets(3, seed=31, out_channels=320)
    tr = ControlNeXtTrainer(nets)              # the reference's defaults (lr 1e-4)
    ref_keys = ["%d.%s" % (i, k) for i in range(3) for k, _ in nets[i].named_parameters()]
    assert list(tr.named_grads()) == ref_keys
    assert set(tr.named_grads()) == set("%d.%s" % (i, k) for i in range(3) for k in nets[i].state_dict())
    hint = rb(torch.rand((2, 3, 128, 128), generator=torch.Generator().manual_seed(32)) * 2 - 1).to(DEV)
    target = [bf(seeded((2, 8, 8, 320), 33 + i, 0.5)).to(DEV) for i in range(3)]
    t = torch.tensor([700.0], device=DEV)
    losses = []
    for _ in range(6):
        outs = tr.forward(hint, t)
        losses.append(sum(((o.float() - y.float()) ** 2).mean().item() for o, y in zip(outs, target)))
        tr.backward([(2.0 / o.numel() * (o.float() - y.float())).to(torch.bfloat16) for o, y in zip(outs, target)])
        tr.step()
    print("losses", losses)
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    path = str(tmp_path / "cn.pt")
    checkpoints.save_control_nets(nets, path)
    back = checkpoints.load_control_nets(path, device=DEV)
    for a, b in zip(nets, back):
        sa, sb = a.state_dict(), b.state_dict()
        assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)
