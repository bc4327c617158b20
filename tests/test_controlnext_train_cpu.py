"""ControlNeXt backward without a GPU: the host-side data-gradient repacks of x2i_amd/lightcontrol_train.py, run through F.conv2d on the CPU, equal
torch.nn.grad.conv2d_input of the original convolution in float64 (odd and even edges of the stride-2 phases included); the new entry points reject
bad arguments with error codes and their workspace queries return the expected sizes."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from tests.util import seeded
from x2i_amd import lightcontrol_train as LT

X2I_ERR_ARG, X2I_ERR_SHAPE, X2I_ERR_ALIGN = -1, -2, -3


def _conv_packed(dy, packed, kh, kw, co, pad_lrtb):
    """the conv of dY (NCHW float64) with a packed [Cout', KH KW Cin'] weight ((ky, kx, ci) order), stride 1, explicit padding"""
    w = packed.view(packed.shape[0], kh, kw, co).permute(0, 3, 1, 2)
    return F.conv2d(F.pad(dy, pad_lrtb), w)


@pytest.mark.parametrize("ci,co,H,W", [(4, 6, 7, 9), (8, 8, 6, 5)])
def test_3x3_repack_is_the_input_gradient(ci, co, H, W):
    w = seeded((co, ci, 3, 3), 1).double()
    dy = seeded((2, co, H, W), 2).double()
    got = _conv_packed(dy, LT.dgrad_weight_3x3(w), 3, 3, co, (1, 1, 1, 1))
    assert torch.allclose(got, torch.nn.grad.conv2d_input((2, ci, H, W), w, dy, padding=1), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("oh,ow", [(4, 5), (5, 3), (1, 1)])
def test_stride2_phases_are_the_input_gradient(oh, ow):
    ci, co = 3, 5
    w = seeded((co, ci, 3, 3), 3).double()
    dy = seeded((2, co, oh, ow), 4).double()
    want = torch.nn.grad.conv2d_input((2, ci, 2 * oh, 2 * ow), w, dy, stride=2, padding=1)
    got = torch.empty_like(want)
    for (py, px), (wp, kh, kw) in LT.dgrad_weights_s2(w).items():
        # pad-0 conv on the dY grid, zero beyond its last row / column (the conv kernel's out_h / out_w)
        got[:, :, py::2, px::2] = _conv_packed(dy, wp, kh, kw, co, (0, kw - 1, 0, kh - 1))
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)


def test_1x1_repack_is_the_input_gradient():
    w = seeded((6, 4, 1, 1), 5).double()
    dy = seeded((2, 6, 5, 7), 6).double()
    got = _conv_packed(dy, LT.dgrad_weight_1x1(w), 1, 1, 6, (0, 0, 0, 0))
    assert torch.allclose(got, torch.nn.grad.conv2d_input((2, 4, 5, 7), w, dy), rtol=1e-12, atol=1e-12)


def test_2x2_stride2_repack_is_the_input_gradient():
    ci, co, ho, wo = 3, 7, 4, 5
    w = seeded((co, ci, 2, 2), 7).double()
    dy = seeded((2, co, ho, wo), 8).double()
    want = torch.nn.grad.conv2d_input((2, ci, 2 * ho, 2 * wo), w, dy, stride=2)
    got = torch.empty_like(want)
    rows = dy.permute(0, 2, 3, 1)                                    # [B, ho, wo, co]
    for ky, wt in enumerate(LT.dgrad_weights_2x2s2(w)):
        pix = (rows @ wt.t()).view(2, ho, wo, 2, ci)                 # [.., kx, ci]: input pixels (2y + ky, 2x + kx)
        got[:, :, ky::2, :] = pix.permute(0, 4, 1, 2, 3).reshape(2, ci, ho, 2 * wo)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)


def _q(fn, *args):
    n = C.c_int64(-7)
    rc = fn(*args, C.byref(n))
    return rc, n.value


def test_workspace_queries_return_the_expected_sizes():
    from x2i_amd import _lib
    lib = _lib.load()
    for B, OH, OW, Cin, Cout, k in [(1, 512, 512, 64, 64, 3), (2, 256, 256, 128, 256, 3), (2, 64, 64, 256, 3072, 2), (3, 7, 5, 128, 128, 1)]:
        rc, n = _q(lib.x2i_conv_wgrad_workspace_floats, B, OH, OW, Cin, Cout, k, k)
        assert rc == 0
        nblk = (Cout // 64) * (Cin // 64) * k * k
        steps = math.ceil(B * OH * OW / 32)
        ns = max(1, min(math.ceil(1024 / nblk), math.ceil(steps / 8)))
        per = math.ceil(steps / ns)
        assert n == math.ceil(steps / per) * (Cout * Cin * k * k + Cout)
    assert _q(lib.x2i_conv_wgrad_workspace_floats, 1, 8, 8, 48, 64, 3, 3)[0] == X2I_ERR_SHAPE
    assert lib.x2i_conv_wgrad_workspace_floats(1, 8, 8, 64, 64, 3, 3, None) == X2I_ERR_ARG
    rc, n = _q(lib.x2i_conv_stem_wgrad_workspace_floats, 2, 1024, 1024, 64)
    assert rc == 0 and n == 1024 * 64 * 28
    assert _q(lib.x2i_conv_stem_wgrad_workspace_floats, 1, 2, 2, 64)[1] == 1 * 64 * 28
    assert _q(lib.x2i_conv_stem_wgrad_workspace_floats, 1, 8, 8, 96)[0] == X2I_ERR_SHAPE
    for B, HW, Cc, G in [(2, 512 * 512, 128, 4), (1, 64 * 64, 256, 8), (3, 100, 64, 2)]:
        rc, n = _q(lib.x2i_groupnorm_bwd_workspace_floats, B, HW, Cc, G)
        nch = max(1, min(math.ceil(1024 / B), math.ceil(HW / 64)))
        nch = math.ceil(HW / math.ceil(HW / nch))
        assert rc == 0 and n == B * nch * 2 * Cc + 2 * B * 2 * Cc + B * G * 4
    assert _q(lib.x2i_groupnorm_bwd_workspace_floats, 1, 64, 128, 3)[0] == X2I_ERR_SHAPE    # C % G
    assert _q(lib.x2i_groupnorm_bwd_workspace_floats, 1, 64, 12, 2)[0] == X2I_ERR_SHAPE     # C % 8


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    from x2i_amd import _lib
    lib = _lib.load()
    f = 0x10000                       # never dereferenced: every call below fails validation first
    big = 1 << 40
    cw = lib.x2i_conv_wgrad_bf16
    # (x, dy, dy_bs, ldy, dw, db, B, H, W, Cin, OH, OW, Cout, KH, KW, stride, pad, accumulate, ws, ws_floats, stream)
    assert cw(None, f, 0, 64, f, f, 1, 8, 8, 64, 8, 8, 64, 3, 3, 1, 1, 0, f, big, None) == X2I_ERR_ARG
    assert cw(f, f, 0, 64, f, f, 1, 8, 8, 64, 8, 8, 64, 3, 3, 1, 1, 0, None, big, None) == X2I_ERR_ARG
    assert cw(f, f, 0, 96, f, f, 1, 8, 8, 96, 8, 8, 64, 3, 3, 1, 1, 0, f, big, None) == X2I_ERR_SHAPE          # Cin % 64
    assert cw(f, f, 0, 64, f, f, 1, 8, 8, 64, 9, 8, 64, 3, 3, 1, 1, 0, f, big, None) == X2I_ERR_SHAPE          # window leaves the input
    assert cw(f, f, 0, 60, f, f, 1, 8, 8, 64, 8, 8, 64, 3, 3, 1, 1, 0, f, big, None) == X2I_ERR_ALIGN          # ldy < Cout
    assert cw(f, f, 4, 72, f, f, 2, 8, 8, 64, 8, 8, 64, 3, 3, 1, 1, 0, f, big, None) == X2I_ERR_ALIGN          # batch stride % 8
    assert cw(f + 8, f, 0, 64, f, f, 1, 8, 8, 64, 8, 8, 64, 3, 3, 1, 1, 0, f, big, None) == X2I_ERR_ALIGN      # 16-byte alignment
    assert cw(f, f, 0, 64, f, f, 1, 8, 8, 64, 8, 8, 64, 3, 3, 1, 1, 0, f, 10, None) == X2I_ERR_ARG             # workspace too small
    assert b"workspace" in lib.x2i_last_error()
    sw = lib.x2i_conv_stem_wgrad_bf16
    assert sw(f, None, f, f, 1, 8, 8, 64, 0, f, big, None) == X2I_ERR_ARG
    assert sw(f, f, f, f, 1, 8, 8, 80, 0, f, big, None) == X2I_ERR_SHAPE
    assert sw(f, f, f, f, 1, 8, 8, 64, 0, f, 1, None) == X2I_ERR_ARG
    gb = lib.x2i_groupnorm_nhwc_bwd_bf16
    # (x, dy, w, b, pre_add, dx, dx_in, dw, db, dpre, B, HW, C, G, eps, act, in_relu, accumulate, ws, ws_floats, stream)
    assert gb(f, f, f, f, None, None, None, f, f, None, 1, 64, 128, 4, 1e-6, 3, 0, 0, f, big, None) == X2I_ERR_ARG    # no dx
    assert gb(f, f, f, f, None, f, None, f, None, None, 1, 64, 128, 4, 1e-6, 3, 0, 0, f, big, None) == X2I_ERR_ARG    # dw without db
    assert gb(f, f, f, f, None, f, None, f, f, None, 1, 64, 128, 4, 1e-6, 1, 0, 0, f, big, None) == X2I_ERR_ARG       # GELU
    assert gb(f, f, f, f, f, f, None, f, f, None, 1, 64, 128, 4, 1e-6, 3, 1, 0, f, big, None) == X2I_ERR_ARG          # in_relu + pre_add
    assert gb(f, f, f, f, None, f, None, f, f, f, 1, 64, 128, 4, 1e-6, 3, 0, 0, f, big, None) == X2I_ERR_ARG          # dpre without pre_add
    assert gb(f, f, f, f, None, f, None, f, f, None, 1, 64, 128, 3, 1e-6, 3, 0, 0, f, big, None) == X2I_ERR_SHAPE     # C % G
    assert gb(f, f + 4, f, f, None, f, None, f, f, None, 1, 64, 128, 4, 1e-6, 3, 0, 0, f, big, None) == X2I_ERR_ALIGN
    assert gb(f, f, f, f, None, f, None, f, f, None, 1, 64, 128, 4, 1e-6, 3, 0, 0, f, 16, None) == X2I_ERR_ARG        # workspace too small
    lw = lib.x2i_linear_wgrad_f32
    assert lw(None, f, f, f, 2, 256, 128, 0, 0, None) == X2I_ERR_ARG
    assert lw(f, f, f, f, 0, 256, 128, 0, 0, None) == X2I_ERR_SHAPE
    assert lw(f, f, f, f, 2, 256, 128, 4, 0, None) == X2I_ERR_ARG                                                   # ReLU input activation


def test_trainer_names_follow_the_module_list_and_step_needs_a_forward():
    """Built on the CPU device: the flat-buffer bookkeeping needs no launch."""
    from x2i_amd.lightcontrol import ControlNeXtModel
    nets = [ControlNeXtModel(device="cpu", control_out_channels=320) for _ in range(2)]
    tr = LT.ControlNeXtTrainer(nets)
    want = ["%d.%s" % (i, k) for i in range(2) for k, _ in nets[i].named_parameters()]
    assert list(tr.named_grads()) == want and "0.embedding.0.weight" in want
    assert tr.grad.numel() == sum(p.numel() for n in nets for p in n.parameters())
    assert all(tr.named_grads()[k].shape == p.shape for k, p in zip(want, tr.params))
    with pytest.raises(RuntimeError):
        tr.backward([None, None])


def test_projector_trainer_exposes_the_same_flat_buffer_bookkeeping():
    """ProjectorTrainer and ControlNeXtTrainer share FlatAdamW; built on the CPU device, no launch."""
    from x2i_amd.proj import Proj7Exp
    from x2i_amd.train import ProjectorTrainer
    pr = Proj7Exp(in_channels=3, input_dim=16, output_dim0=8, output_dim1=24, use_t5=False, use_scale=False, use_cnn=True, device="cpu")
    tr = ProjectorTrainer(pr)
    named = list(pr.named_parameters())
    assert tr.names == [n for n, _ in named] and "conv.weight" in tr.names
    assert all(a is b for a, (_, b) in zip(tr.params, named))
    o = 0
    for n, p in named:
        assert tr.off[n] == (o, p.numel()) and tr.g(n).numel() == p.numel() and tr.g(n).data_ptr() == tr.grad.data_ptr() + 4 * o
        o += p.numel()
    assert o == tr.grad.numel() == tr.m.numel() == tr.v.numel() and tr.grad.dtype == torch.float32
    assert list(tr.named_grads()) == tr.names and tr.step_count == 0 and tr.last_norm is None
