"""Every convolution and GroupNorm kernel against the float64 reference of tests/conv_ref.py -- every output element of every launch, the
sentinel outside what the launch may write, every entry of the epilogue moments.

(a) Unit launches of x2i_conv2d_nhwc_bf16, per kernel form.  `last_gemm_tile` is read after every launch and asserted: 5256 = the persistent
    four-wave 256^2 kernel (gemm256c.hip), 5512 = the persistent 512 x 128 kernel (gemm512c.hip), 256 = the eight-wave 256^2 kernel, 128 = the
    128^2 kernel.  Every case runs under conv_w4 1 / 0 and conv_korder 1 (the product's K order) / 0, with gemm_min256 = 1 (the item threshold of
    the 256-wide forms lowered to test-sized images), on every operand kind of conv_ref.CONV_KINDS.  The fused-upsample gathers (up = 1, up = 2)
    are not taken by the persistent kernels: they run on the eight-wave 256^2 kernel (Cout >= 256, M >= 1024) or the 128^2 kernel, under either
    setting of conv_w4.  Shapes: the smallest at which a form is still taken (M >= 1024 for the 256-wide forms, M >= 2048 for 512 x 128) with a
    ragged last tile and an image width (80, 56, 40) that does not divide the tile rows, so image rows and batch items straddle tiles.
(b) x2i_conv3x3_narrow_bf16, x2i_conv3x3_image_bf16 (with and without moments), x2i_conv_stem_bf16.
(c) x2i_groupnorm_nhwc*_bf16, x2i_groupnorm_moments_f32, x2i_groupnorm_nhwc_from_moments*_bf16 on every operand kind of conv_ref.GN_KINDS.  For
    the kinds random / outlier / pre_add_dominant the f32 part of the bound is a small fraction of the output's own rounding (asserted from the
    reference alone, before the kernel's output is looked at: median delta / (ulp / 2) < 1 %): there the check is a one-rounding check.  For
    large_mean and const the derived bound is loose; they assert the bound, finiteness and the clamp of the variance; their
    share is reported only.
(d) The launch lists of the models, recorded with the seven ops functions replaced by a recorder (reduced-width VAE decode and encode,
    ControlNeXt forward in the chained form and as a grouped bank of 3 nets, one ControlNeXtTrainer backward; 128^2 hint, B = 2), asserted in
    order, and every launch replayed with its recorded geometry (every shape, stride, offset, ldc, row pitch, aliasing) on fresh poisoned
    storages, once with the thresholds the model ran under and once with gemm_min256 = 1 (the kernels a 1024^2 image takes).
(e) Negative controls: a real kernel output against a deliberately wrong expectation must be rejected at the expected sample, pixel and channel.

Out of scope: the 2 GB chunking of launch_conv_chunks (csrc/gemm.hip) cannot be reached at these sizes.

The largest share of the f32 allowance used per launch kind and kernel form is kept in WORST and printed at the end of each test; FORMS is the
table of kernel forms met."""
import inspect
import math
import time

import pytest
import torch

from tests import conv_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}      # launch kind / kernel form -> worst share of the f32 allowance used, over everything this module ran
FORMS = {}      # (group, launch) -> {(conv_w4, conv_korder, gemm_min256): last_gemm_tile}
KAPPA = {}      # recording -> {operand kind: largest finite kappa met in its GroupNorm replays}
DEFAULTS = dict(conv_w4=1, conv_korder=1, gemm_min256=128)
CONFIGS = [(1, 1), (1, 0), (0, 1), (0, 0)]      # (conv_w4, conv_korder)


@pytest.fixture(scope="module")
def ops():
    from x2i_amd import ops as o
    o._lib.load()
    return o


def note(name, share):
    WORST[name] = max(WORST.get(name, 0.0), share)


def print_worst(label, t0):
    print(f"\n  {label} ({time.time() - t0:.1f} s); worst share of the f32 allowance: " +
          ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


class options:
    """conv_w4 / conv_korder / gemm_min256 for the duration of a block; the defaults come back however it ends"""

    def __init__(self, ops, **kw):
        self.lib, self.kw = ops._lib, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.lib.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            self.lib.set_option(k, DEFAULTS[k])
        return False


def form_key(tile, korder):
    return f"{tile}/k{korder}" if tile > 5000 else str(tile)


# ---------------------------------------------------------------------------------------------------------------- one conv launch
def cp(Cin, Cout, KH, KW, stride, pad, H, W, B, **kw):
    """geometry of one x2i_conv2d_nhwc_bf16 launch.  res: None / "sep" (a storage of its own) / "alias" (the output storage); moments: None /
    "plain" / "acc"; x_numel / out_numel / res_numel: sizes of the storages when they are larger than the launch needs"""
    p = dict(Cin=Cin, Cout=Cout, KH=KH, KW=KW, stride=stride, pad=pad, H=H, W=W, B=B, act=R.ACT_NONE, up=0, pad_w=None, out_w=None, out_h=None,
             out_row_pitch=0, c_offset=0, c_batch_stride=None, ldc=None, res=None, res_offset=0, res_batch_stride=None, ldr=None, a_offset=0,
             a_batch_stride=None, bias=True, bias2=False, w_group=0, moments="plain", x_numel=None, out_numel=None, res_numel=None)
    assert not set(kw) - set(p), set(kw) - set(p)
    p.update(kw)
    return p


def geom(p):
    return R.Geom(p["H"], p["W"], p["Cin"], p["KH"], p["KW"], p["stride"], p["pad"], up=p["up"], pad_w=p["pad_w"], out_w=p["out_w"],
                  out_h=p["out_h"])


def out_view(p):
    return R.out_geometry(geom(p), p["Cout"], p["B"], c_offset=p["c_offset"], c_batch_stride=p["c_batch_stride"], ldc=p["ldc"],
                          out_row_pitch=p["out_row_pitch"])


def out_extent(p):
    """elements of the output storage up to the last one the launch may write"""
    shape, stride, off = out_view(p)
    return off + sum((s - 1) * t for s, t in zip(shape, stride)) + 1


def _noise(n, kind, gen):
    t = torch.randn(n, device=DEV, generator=gen)
    return ((t + 4.0) if kind == "cancel" else t).to(torch.bfloat16)


class State:
    pass


def conv_state(p, kind, seed, share=None):
    """operands and storages of one launch; share: a State whose input and output storages this launch uses too (several launches, one buffer)"""
    g, N, B = geom(p), p["Cout"], p["B"]
    gen = torch.Generator(device=DEV).manual_seed(seed)
    st = State()
    x, st.w, bias = R.conv_operands(kind, B, p["H"], p["W"], p["Cin"], N, p["KH"], p["KW"], gen, DEV, groups=B // p["w_group"] if p["w_group"] else 0)
    st.bias = bias if p["bias"] else None
    st.bias2 = 0.5 * torch.randn((B, N), device=DEV, generator=gen) if p["bias2"] else None
    if share is not None:
        st.x, st.out = share.x, share.out
        assert out_extent(p) <= st.out.numel()
    else:
        item = p["H"] * p["W"] * p["Cin"]
        abs_ = item if p["a_batch_stride"] is None else p["a_batch_stride"]
        st.x = _noise(max(p["a_offset"] + (B - 1) * abs_ + item, p["x_numel"] or 0), kind, gen)
        for z in range(B):
            R.item_view(st.x, g, z, p["a_offset"], p["a_batch_stride"]).copy_(x[z])
        st.out = R.poison_(torch.empty(max(out_extent(p) + 72, p["out_numel"] or 0), device=DEV, dtype=torch.bfloat16))
    del x
    st.res_t = st.res_store = None
    if p["res"] is not None:
        ldr = N if p["ldr"] is None else p["ldr"]
        rbs = g.M * N if p["res_batch_stride"] is None else p["res_batch_stride"]
        rview = ((B, g.M, N), (rbs, ldr, 1), p["res_offset"])
        if p["res"] == "alias":
            st.res_t = st.out
            st.out.as_strided(*rview).copy_(torch.randn((B, g.M, N), device=DEV, generator=gen).to(torch.bfloat16))
            st.res_store = st.out.clone()
        else:
            need = p["res_offset"] + (B - 1) * rbs + (g.M - 1) * ldr + N
            st.res_t = st.res_store = torch.randn(max(need, p["res_numel"] or 0), device=DEV, generator=gen).to(torch.bfloat16)
    st.mom = st.prev = None
    if p["moments"] is not None:
        if share is not None and p["moments"] == "acc":
            st.mom = share.mom
        elif p["moments"] == "acc":
            st.mom = (100.0 * torch.randn((B, N, 2), device=DEV, generator=gen)).contiguous()
        else:
            st.mom = torch.full((B, N, 2), 7.0, device=DEV)
    return st


def conv_launch(ops, p, st):
    if st.mom is not None:
        st.prev = st.mom.clone()
    ops.conv2d_nhwc(st.x, st.w, st.bias, p["H"], p["W"], p["Cin"], p["Cout"], p["KH"], p["KW"], p["stride"], p["pad"], out=st.out, act=p["act"],
                    bias2=st.bias2, res=st.res_t, c_offset=p["c_offset"], c_batch_stride=p["c_batch_stride"], ldc=p["ldc"],
                    res_offset=p["res_offset"], res_batch_stride=p["res_batch_stride"], ldr=p["ldr"], up=p["up"], pad_w=p["pad_w"], B=p["B"],
                    a_batch_stride=p["a_batch_stride"], a_offset=p["a_offset"], out_w=p["out_w"], out_h=p["out_h"],
                    out_row_pitch=p["out_row_pitch"], moments=st.mom, moments_accumulate=p["moments"] == "acc", w_group=p["w_group"])
    torch.cuda.synchronize()
    return int(ops._lib.get_option("last_gemm_tile"))


def conv_check_output(p, st, name, rep=None):
    rep = R.Report(name) if rep is None else rep
    R.check_conv(rep, st.x, st.w, st.bias, st.out, geom(p), p["Cout"], p["B"], act=p["act"], bias2=st.bias2, res_store=st.res_store,
                 res_offset=p["res_offset"], res_batch_stride=p["res_batch_stride"], ldr=p["ldr"], w_group=p["w_group"], a_offset=p["a_offset"],
                 a_batch_stride=p["a_batch_stride"], c_offset=p["c_offset"], c_batch_stride=p["c_batch_stride"], ldc=p["ldc"],
                 out_row_pitch=p["out_row_pitch"])
    return rep.done()


def conv_check_moments(p, st, tile, name):
    """every entry of the moments buffer after the launch: the sums of the STORED outputs of this launch (+ the buffer's contents before it)"""
    g, N, B = geom(p), p["Cout"], p["B"]
    Y = st.out.as_strided(*out_view(p)).reshape(B, g.M, N)
    acc = p["moments"] == "acc"
    depth = R.moments_depth(g.M, N, 64 if tile == 128 else 128, accumulate=acc, blocks=(g.M + 511) // 512 * 4 if tile == 5512 else None)
    want, bound = R.moments_expect(Y, depth, prev=st.prev if acc else None)
    return R.assert_entries(f"{name} moments", st.mom, want, bound)


def run_conv(ops, p, kind, seed, name, korder=1):
    """one launch on fresh poisoned storages, checked whole: (tile, share of the output allowance, share of the moments allowance or None)"""
    st = conv_state(p, kind, seed)
    tile = conv_launch(ops, p, st)
    share = conv_check_output(p, st, name)
    R.check_untouched(name, st.out, R.write_mask(st.out, [out_view(p)]))
    note(f"conv {form_key(tile, korder)}", share)
    ms = None
    if st.mom is not None:
        ms = conv_check_moments(p, st, tile, name)
        note(f"moments {form_key(tile, korder)}", ms)
    return tile, share, ms


# ---------------------------------------------------------------------------------------------------------------- (a) unit launches
RELU = R.ACT_RELU
UNIT = [
    # label, geometry, form under conv_w4 = 1, form under conv_w4 = 0 (both with gemm_min256 = 1)
    # ---- Cout >= 256: the 256^2 forms
    ("3x3 128>256 48x80 B3", cp(128, 256, 3, 3, 1, 1, 48, 80, 3), 5256, 256),              # M = 3840 = 15 tiles; rows of 80 straddle the tiles
    ("3x3 512>512 32x40", cp(512, 512, 3, 3, 1, 1, 32, 40, 2), 5256, 256),                 # Cin = 512; M = 1280: a ragged fifth tile
    ("3x3 256>320 40x40", cp(256, 320, 3, 3, 1, 1, 40, 40, 2), 5256, 256),                 # N = 320: the second tile column partly out of range
    ("3x3s2 128>256 72x80", cp(128, 256, 3, 3, 2, 1, 72, 80, 2), 5256, 256),               # Downsample2D: 36 x 40 outputs, M = 1440
    ("5x5s2 128>256 80x112", cp(128, 256, 5, 5, 2, 2, 80, 112, 2), 5256, 256),             # the composed chain: 25 taps; 40 x 56, M = 2240
    ("2x2s2 256>3072 64x80", cp(256, 3072, 2, 2, 2, 0, 64, 80, 2, moments=None), 5256, 256),   # ControlNeXt's last conv: N = 3072, M = 1280
                                                                                           # (the epilogue moments serve N <= 2048)
    ("3x3 64>256 40x56", cp(64, 256, 3, 3, 1, 1, 40, 56, 2), 5256, 256),                   # Cin = 64: the tap advances on every K-tile
    ("1x1 256>256 40x40", cp(256, 256, 1, 1, 1, 0, 40, 40, 2), 5256, 256),                 # four K-tiles, M = 1600
    ("relu+bias2 256", cp(128, 256, 3, 3, 1, 1, 32, 40, 2, act=RELU, bias2=True), 5256, 256),
    ("no bias 256", cp(128, 256, 3, 3, 1, 1, 32, 40, 2, bias=False), 5256, 256),
    ("res 256 (trainer dgrad 3x3 + res)", cp(256, 256, 3, 3, 1, 1, 32, 40, 2, res="sep", bias=False), 5256, 256),
    ("res aliasing out 256", cp(128, 256, 3, 3, 1, 1, 32, 40, 2, res="alias"), 5256, 256),
    ("res_batch_stride 0, 3x3s2 128>256", cp(128, 256, 3, 3, 2, 1, 72, 80, 2, res="sep", res_batch_stride=0, bias=False), 5256, 256),
    ("grouped 256 B6 w_group 2", cp(128, 256, 3, 3, 1, 1, 32, 40, 6, w_group=2), 5256, 256),
    ("up=1 3x3 128>256 16x40", cp(128, 256, 3, 3, 1, 1, 16, 40, 2, up=1), 256, 256),       # fused upsample: 32 x 80 outputs, the eight-wave kernel
    # ---- 64 < Cout <= 128: the 512 x 128 form against the 128^2 kernel
    ("3x3 256>128 48x80", cp(256, 128, 3, 3, 1, 1, 48, 80, 2), 5512, 128),                 # M = 3840: 7.5 tiles of 512
    ("3x3 128>96 56x40", cp(128, 96, 3, 3, 1, 1, 56, 40, 2), 5512, 128),                   # N = 96: the tile's last 32 columns out of range; M = 2240
    ("5x5s2 128>128 96x112", cp(128, 128, 5, 5, 2, 2, 96, 112, 2), 5512, 128),             # 48 x 56, M = 2688
    ("3x3s2 128>128 96x112", cp(128, 128, 3, 3, 2, 1, 96, 112, 2), 5512, 128),
    ("1x1 256>128 56x40 (trainer dgrad 1x1)", cp(256, 128, 1, 1, 1, 0, 56, 40, 2, bias=False), 5512, 128),
    ("3x3 64>128 56x40", cp(64, 128, 3, 3, 1, 1, 56, 40, 2), 5512, 128),
    ("3x3 512>128 56x40", cp(512, 128, 3, 3, 1, 1, 56, 40, 1), 5512, 128),
    ("2x2s2 128>128 112x80", cp(128, 128, 2, 2, 2, 0, 112, 80, 2), 5512, 128),
    ("relu+bias2 128", cp(128, 128, 3, 3, 1, 1, 56, 40, 2, act=RELU, bias2=True), 5512, 128),
    ("res 128 (trainer dgrad 3x3 + res)", cp(128, 128, 3, 3, 1, 1, 56, 40, 2, res="sep", bias=False), 5512, 128),
    ("res aliasing out 128", cp(128, 128, 3, 3, 1, 1, 56, 40, 2, res="alias"), 5512, 128),
    ("res_batch_stride 0, 3x3s2 128>128", cp(128, 128, 3, 3, 2, 1, 96, 112, 2, res="sep", res_batch_stride=0, bias=False), 5512, 128),
    ("grouped 128 B6 w_group 2", cp(128, 128, 3, 3, 1, 1, 56, 40, 6, w_group=2), 5512, 128),
    ("up=1 3x3 128>128 16x40", cp(128, 128, 3, 3, 1, 1, 16, 40, 2, up=1), 128, 128),
    # ---- the 128^2 kernel alone
    ("3x3 64>64 24x40", cp(64, 64, 3, 3, 1, 1, 24, 40, 2), 128, 128),                      # ControlNeXt's embedding conv
    ("3x3 128>256 16x40 (M < 1024)", cp(128, 256, 3, 3, 1, 1, 16, 40, 3), 128, 128),
    # the strip convs of lightcontrol._composed_apply: a window of a larger input (B, a_batch_stride, a_offset), H = 1 / W = 1, the result added
    # into the first row / column of the output in place (res aliasing out)
    ("strip 1x5 s2, H = 1, in place", cp(128, 128, 1, 5, 2, 0, 1, 48, 2, pad_w=2, a_batch_stride=32 * 48 * 128, x_numel=2 * 32 * 48 * 128,
                                         c_batch_stride=16 * 24 * 128, out_numel=2 * 16 * 24 * 128, res="alias",
                                         res_batch_stride=16 * 24 * 128, bias=False, moments=None), 128, 128),
    ("strip 1x5 s2, H = 1, a_offset", cp(128, 256, 1, 5, 2, 0, 1, 48, 3, pad_w=2, a_offset=5 * 48 * 128, a_batch_stride=32 * 48 * 128,
                                         x_numel=3 * 32 * 48 * 128, c_batch_stride=16 * 24 * 256, out_numel=3 * 16 * 24 * 256, res="alias",
                                         res_batch_stride=16 * 24 * 256, bias=False, moments=None), 128, 128),
    ("strip 5x1 s2, W = 1, in place", cp(256, 256, 5, 1, 2, 2, 32, 1, 2, pad_w=0, c_batch_stride=16 * 24 * 256, ldc=24 * 256,
                                         out_numel=2 * 16 * 24 * 256, res="alias", res_batch_stride=16 * 24 * 256, ldr=24 * 256, bias=False,
                                         moments=None), 128, 128),
]


@pytest.mark.parametrize("label,p,form_new,form_old", UNIT, ids=[u[0] for u in UNIT])
def test_conv_unit_launches_vs_fp64(ops, label, p, form_new, form_old):
    t0 = time.time()
    row = FORMS.setdefault(("unit", label), {})
    for w4, korder in CONFIGS:
        with options(ops, conv_w4=w4, conv_korder=korder, gemm_min256=1):
            for j, kind in enumerate(R.CONV_KINDS):
                tile, share, ms = run_conv(ops, p, kind, 100 * j + 7, f"{label} w4={w4} korder={korder} {kind}", korder)
                assert tile == (form_new if w4 else form_old), (label, w4, korder, tile)
                row[(w4, korder, 1)] = tile
    print(f"\n  {label}: forms {row}")
    print_worst(label, t0)


def _vae_phases(C, Co, H, W, B=2):
    """the four 2 x 2 phase launches of Upsample2D's conv (vae._Conv.packed_up_phases(rows=True)), moments accumulated over them"""
    return [cp(C, Co, 2, 2, 1, 1 - py, H, W, B, pad_w=1 - px, out_w=W, out_h=H, ldc=2 * Co, out_row_pitch=4 * W * Co,
               c_offset=(py * 2 * W + px) * Co, c_batch_stride=4 * H * W * Co, moments="plain" if (py, px) == (0, 0) else "acc")
            for py in (0, 1) for px in (0, 1)]


def _column_phases(C, Co, H, W, B=2):
    """the two 3 x 2 column-phase launches (x2i_conv_desc.up = 2: rows doubled in the gather), moments accumulated"""
    return [cp(C, Co, 3, 2, 1, 1, H, W, B, up=2, pad_w=1 - px, out_w=W, ldc=2 * Co, c_offset=px * Co, c_batch_stride=4 * H * W * Co,
               moments="acc" if px else "plain") for px in (0, 1)]


def _dgrad_s2_phases(co, ci, oh, ow, B=2):
    """the four phase launches of lightcontrol_train.dgrad_s2: 1x1, 1x2, 2x1, 2x2 stride-1 pad-0 convs on the dY grid, ldc = 2 ci"""
    return [cp(co, ci, 1 + py, 1 + px, 1, 0, oh, ow, B, out_h=oh, out_w=ow, ldc=2 * ci, out_row_pitch=4 * ow * ci,
               c_offset=(py * 2 * ow + px) * ci, c_batch_stride=4 * oh * ow * ci, bias=False, moments=None)
            for py in (0, 1) for px in (0, 1)]


PHASED = [
    # label, launches, form under conv_w4 = 1, under conv_w4 = 0 (gemm_min256 = 1)
    ("vae four phases 256>256 32x40", _vae_phases(256, 256, 32, 40), 5256, 256),
    ("vae four phases 128>128 24x40", _vae_phases(128, 128, 24, 40), 128, 128),            # (a row pitch: not the 512 x 128 kernel)
    ("column phases up=2 128>256 16x40", _column_phases(128, 256, 16, 40), 256, 256),      # M = 1280: the eight-wave kernel
    ("column phases up=2 128>128 16x40", _column_phases(128, 128, 16, 40), 128, 128),
    ("trainer dgrad_s2 256>256 32x40", _dgrad_s2_phases(256, 256, 32, 40), 5256, 256),     # (the 1x1 phase: K = 256, four K-tiles)
    ("trainer dgrad_s2 128>128 24x40", _dgrad_s2_phases(128, 128, 24, 40), 128, 128),
]


def run_phased(ops, launches, kind, seed, name, korder=1):
    """several launches into ONE poisoned buffer: the moments after each launch, every launch's outputs after the last, and the sentinel outside
    the union of the write sets"""
    tiles, states = [], []
    numel = max(out_extent(p) for p in launches) + 72           # one buffer that holds every launch's write set
    for i, p in enumerate(launches):
        st = conv_state(dict(p, out_numel=numel), kind, seed + i, share=states[0] if states else None)
        tile = conv_launch(ops, p, st)
        if st.mom is not None:
            note(f"moments {form_key(tile, korder)}", conv_check_moments(p, st, tile, f"{name} launch {i}"))
        tiles.append(tile)
        states.append(st)
    for i, (p, st, tile) in enumerate(zip(launches, states, tiles)):
        note(f"conv {form_key(tile, korder)}", conv_check_output(p, st, f"{name} launch {i}"))
    R.check_untouched(name, states[0].out, R.write_mask(states[0].out, [out_view(p) for p in launches]))
    return tiles


@pytest.mark.parametrize("label,launches,form_new,form_old", PHASED, ids=[u[0] for u in PHASED])
def test_conv_phase_launches_into_one_buffer_vs_fp64(ops, label, launches, form_new, form_old):
    t0 = time.time()
    row = FORMS.setdefault(("unit", label), {})
    for w4, korder in CONFIGS:
        with options(ops, conv_w4=w4, conv_korder=korder, gemm_min256=1):
            for j, kind in enumerate(R.CONV_KINDS):
                tiles = run_phased(ops, launches, kind, 100 * j + 11, f"{label} w4={w4} korder={korder} {kind}", korder)
                assert tiles == [form_new if w4 else form_old] * len(launches), (label, w4, korder, tiles)
                row[(w4, korder, 1)] = tiles[0]
    print(f"\n  {label}: forms {row}")
    print_worst(label, t0)


@pytest.mark.parametrize("p,form_new,form_old", [(cp(128, 256, 3, 3, 1, 1, 32, 40, 2), 5256, 256), (cp(128, 128, 3, 3, 1, 1, 56, 40, 2), 5512, 128),
                                                 (cp(64, 64, 3, 3, 1, 1, 24, 40, 2), 128, 128)], ids=["256", "128", "64"])
def test_conv_moments_accumulate_over_two_launches(ops, p, form_new, form_old):
    """moments_accumulate: the second launch adds to what the first left; prev is the buffer's content before each launch"""
    t0 = time.time()
    for w4, korder in CONFIGS:
        with options(ops, conv_w4=w4, conv_korder=korder, gemm_min256=1):
            for j, kind in enumerate(R.CONV_KINDS):
                name = f"accumulate w4={w4} korder={korder} {kind}"
                st = conv_state(p, kind, 100 * j + 13)
                assert float(st.mom.abs().min()) == 7.0             # (the buffer starts as a known nonzero value)
                for n, mode in enumerate(("plain", "acc")):
                    q = dict(p, moments=mode)
                    tile = conv_launch(ops, q, st)
                    assert tile == (form_new if w4 else form_old)
                    note(f"moments {form_key(tile, korder)}", conv_check_moments(q, st, tile, f"{name} launch {n}"))
                note(f"conv {form_key(tile, korder)}", conv_check_output(p, st, name))
    print_worst("moments accumulate", t0)


# ---------------------------------------------------------------------------------------------------------------- (b) narrow, image, stem
def run_narrow(ops, B, H, W, Cin, Cout, ldy, kind, seed, name, bias=True):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x, w, b = R.conv_operands(kind, B, H, W, Cin, Cout, 3, 3, gen, DEV)
    buf = R.poison_(torch.empty(B * H * W * ldy + 40, device=DEV, dtype=torch.bfloat16))
    y = buf[:B * H * W * ldy].view(B, H, W, ldy)
    ops.conv3x3_narrow(x, w, b if bias else None, Cout, out=y, ldy=ldy)
    torch.cuda.synchronize()
    rep = R.check_narrow(R.Report(name), x, w, b if bias else None, y, Cout)
    share = rep.done()
    R.check_untouched(name, buf, R.write_mask(buf, [((B, H, W, 4), (H * W * ldy, W * ldy, ldy, 1), 0)]))
    note("conv3x3_narrow", share)
    return share


@pytest.mark.parametrize("H,W", [(37, 29), (5, 11)], ids=["37x29", "5x11"])
@pytest.mark.parametrize("Cout,ldy", [(3, 4), (4, 4), (3, 8)])
def test_conv3x3_narrow_vs_fp64(ops, H, W, Cout, ldy):
    t0 = time.time()
    for j, kind in enumerate(R.CONV_KINDS):
        run_narrow(ops, 2, H, W, 128, Cout, ldy, kind, 100 * j + 17, f"narrow {H}x{W} Cout={Cout} ldy={ldy} {kind}", bias=(j != 1 or Cout != 4))
    print_worst(f"narrow {H}x{W} Cout={Cout}", t0)


def run_image(ops, B, Cin, H, W, Cout, kind, seed, name, moments):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x, w, b = R.conv_operands(kind, B, H, W, Cin, Cout, 3, 3, gen, DEV)
    x_nchw = x.permute(0, 3, 1, 2).contiguous()
    w4 = w.view(Cout, 3, 3, Cin).permute(0, 3, 1, 2).contiguous()          # the nn.Conv2d layout
    mom = torch.full((B, Cout, 2), 7.0, device=DEV) if moments else None
    y = ops.conv3x3_image(x_nchw, w4, b, moments=mom)
    torch.cuda.synchronize()
    assert y.shape == (B, H, W, Cout)
    share = R.check_image(R.Report(name), x_nchw, w4, b, y).done()
    note("conv3x3_image", share)
    if moments:
        want, bound = R.moments_expect(y.reshape(B, H * W, Cout), R.image_moments_depth(H, W, Cout))
        note("moments conv3x3_image", R.assert_entries(f"{name} moments", mom, want, bound))
    return y


@pytest.mark.parametrize("moments", [False, True], ids=["plain", "moments"])
def test_conv3x3_image_vs_fp64(ops, moments):
    t0 = time.time()
    for j, kind in enumerate(R.CONV_KINDS):
        run_image(ops, 2, 3, 40, 24, 128, kind, 100 * j + 19, f"image 40x24 {kind}", moments)
    print_worst("image conv", t0)


def run_stem(ops, B, H, W, Cout, kind, seed, name):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x, w, b = R.conv_operands(kind, B, H, W, 3, Cout, 3, 3, gen, DEV)
    wf, bf_ = w.float().view(Cout, 3, 3, 3).contiguous(), b.float()
    y = ops.conv_stem(x, wf, bf_, Cout)
    torch.cuda.synchronize()
    assert y.shape == (B, H // 2, W // 2, Cout)
    share = R.check_stem(R.Report(name), x, wf, bf_, y).done()
    note("conv_stem", share)
    return share


def test_conv_stem_vs_fp64(ops):
    t0 = time.time()
    for j, kind in enumerate(R.CONV_KINDS):
        run_stem(ops, 2, 38, 50, 64, kind, 100 * j + 23, f"stem 38x50 {kind}")
    print_worst("stem conv", t0)


# ---------------------------------------------------------------------------------------------------------------- (c) GroupNorm
ONE_ROUNDING_KINDS = ("random", "outlier", "pre_add_dominant")


class DryReport(R.Report):
    """collects delta / (half an output ulp) of every element from the REFERENCE alone (the kernel's output is not looked at)"""

    def __init__(self):
        super().__init__("dry")
        self.ratio = []

    def check(self, got, want, bound, delta=None, **kw):
        self.ratio.append((delta / (0.5 * R.ulp_bf16(want))).flatten())

    def median(self):
        return float(torch.cat(self.ratio).median())


def quad_moments(x):
    """channel-quad moments f32 [B, C, 2] of x [B, HW, C], as a conv epilogue leaves them (entries c % 4 != 0 zero)"""
    B, HW, C = x.shape
    q = x.double().reshape(B, HW, C // 4, 4)
    mom = torch.zeros((B, C, 2), device=x.device, dtype=torch.float64)
    mom[:, 0::4, 0], mom[:, 0::4, 1] = q.sum((1, 3)), (q * q).sum((1, 3))
    return mom.float()


def run_gn(ops, B, HW, C, G, kind, seed, name, *, act=R.ACT_NONE, eps=1e-6, pre=False, post=False, form="direct", w_group=0, key=None, one_rounding=True):
    """one GroupNorm launch (form: direct / chan = from groupnorm_moments(x) / quad = from channel-quad moments), checked whole"""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x, pa = R.gn_input(kind, B, HW, C, G, gen, DEV)
    pa = pa.contiguous() if (pre and pa is not None) else None
    w, b = R.gn_affine(C, gen, DEV, groups=B // w_group if w_group else 0)
    pst = torch.randn((B, HW, C), device=DEV, generator=gen).to(torch.bfloat16) if post else None
    buf = R.poison_(torch.empty(B * HW * C + 72, device=DEV, dtype=torch.bfloat16))
    y = buf[:B * HW * C].view(B, HW, C)
    mom = None
    if form == "chan":
        mom = ops.groupnorm_moments(x)
        torch.cuda.synchronize()
        want, bound = R.gn_moments_expect(x)
        note("groupnorm_moments", R.assert_entries(f"{name} groupnorm_moments", mom, want, bound))
    elif form == "quad":
        assert pa is None
        mom = quad_moments(x)
    kw = dict(act=act, pre_add=pa, w_group=w_group)
    ckw = dict(kw, post=pst, moments=mom)
    med = None
    if one_rounding and form == "direct" and kind in ONE_ROUNDING_KINDS:
        dry = DryReport()
        R.check_groupnorm(dry, x, y, w, b, G, eps, **ckw)
        med = dry.median()
        assert med < 0.01, f"{name}: the f32 part of the bound is {med:.4f} of half an output ulp by the median element: not a one-rounding check"
    if form == "direct":
        ops.groupnorm_nhwc(x, w, b, G, eps, post_add=pst, out=y, **kw)
    else:
        ops.groupnorm_nhwc_from_moments(x, mom, w, b, G, eps, post_add=pst, out=y, **kw)
    torch.cuda.synchronize()
    rep = R.Report(name)
    info = R.check_groupnorm(rep, x, y, w, b, G, eps, **ckw)
    share = rep.done()
    assert bool(torch.isfinite(y.float()).all()), name
    R.check_untouched(name, buf, R.write_mask(buf, [((B, HW, C), (HW * C, C, 1), 0)]))
    note(key or f"groupnorm {form} {kind}", share)
    return share, info, med


GN_SHAPES = [(1073, 128, 32), (1920, 256, 8), (1023, 64, 2), (576, 512, 32), (200, 128, 32), (257, 128, 32)]
GN_VARIANTS = [
    dict(act=R.ACT_NONE, eps=1e-6, pre=False, post=False, form="direct"),
    dict(act=R.ACT_SILU, eps=1e-5, pre=True, post=False, form="direct"),
    dict(act=R.ACT_RELU, eps=1e-6, pre=True, post=True, form="direct"),
    dict(act=R.ACT_SILU, eps=1e-6, pre=True, post=False, form="chan"),
    dict(act=R.ACT_RELU, eps=1e-5, pre=False, post=True, form="chan"),
    dict(act=R.ACT_NONE, eps=1e-6, pre=False, post=True, form="quad"),
]


@pytest.mark.parametrize("kind", R.GN_KINDS)
@pytest.mark.parametrize("HW,C,G", GN_SHAPES, ids=[f"{s[0]}x{s[1]}g{s[2]}" for s in GN_SHAPES])
def test_groupnorm_vs_fp64(ops, HW, C, G, kind):
    t0 = time.time()
    lines = []
    for j, v in enumerate(GN_VARIANTS):
        share, info, med = run_gn(ops, 2, HW, C, G, kind, 1000 * j + HW, f"gn HW={HW} C={C} G={G} {kind} {v}", **v)
        lines.append(f"{v['form']} act={v['act']} eps={v['eps']:g} pre={int(v['pre'])} post={int(v['post'])}: share {share:.3f}, kappa "
                     f"{info['kappa']:.3g}" + (f", median delta / (ulp / 2) {med:.4f}" if med is not None else ""))
    print(f"\n  gn HW={HW} C={C} G={G} {kind}:\n    " + "\n    ".join(lines))
    print_worst(f"gn HW={HW} C={C} G={G} {kind}", t0)


@pytest.mark.parametrize("kind", ["random", "const", "pre_add_dominant"])
def test_groupnorm_grouped_weights_vs_fp64(ops, kind):
    """w_group: B = 6, item b takes weight / bias row b // 2"""
    t0 = time.time()
    for j, v in enumerate(GN_VARIANTS[1:5]):
        run_gn(ops, 6, 257, 128, 32, kind, 1000 * j + 3, f"gn grouped {kind} {v}", w_group=2, **v)
    print_worst(f"gn grouped {kind}", t0)


def test_groupnorm_from_conv_epilogue_moments_vs_fp64(ops):
    """the from-moments form on the channel-quad moments a conv epilogue wrote: the moments GIVEN are the operand"""
    t0 = time.time()
    for p, G in ((cp(128, 256, 3, 3, 1, 1, 32, 40, 2), 32), (cp(128, 128, 3, 3, 1, 1, 24, 40, 2), 32)):
        for gm in (1, 128):
            with options(ops, gemm_min256=gm):
                st = conv_state(p, "random", 29)
                tile = conv_launch(ops, p, st)
                conv_check_moments(p, st, tile, f"conv for gn, tile {tile}")
            B, HW, C = p["B"], p["H"] * p["W"], p["Cout"]
            x = st.out[:B * HW * C].view(B, HW, C).clone()
            gen = torch.Generator(device=DEV).manual_seed(31)
            w, b = R.gn_affine(C, gen, DEV)
            y = R.poison_(torch.empty_like(x))
            ops.groupnorm_nhwc_from_moments(x, st.mom, w, b, G, 1e-6, act=R.ACT_SILU, out=y)
            torch.cuda.synchronize()
            rep = R.Report(f"gn from the epilogue moments of tile {tile}")
            R.check_groupnorm(rep, x, y, w, b, G, 1e-6, act=R.ACT_SILU, moments=st.mom, W=p["W"])
            note("groupnorm quad (conv epilogue)", rep.done())
    print_worst("gn from conv epilogue moments", t0)


# ---------------------------------------------------------------------------------------------------------------- (d) recordings
WRAPPED = ("conv2d_nhwc", "conv3x3_narrow", "conv3x3_image", "conv_stem", "groupnorm_nhwc", "groupnorm_moments", "groupnorm_nhwc_from_moments")
CONV, NARROW, IMAGE, STEM, GN, GNM, GNF = WRAPPED


class Spec:
    """geometry of one tensor argument: its storage (identity and size in elements), dtype, shape, strides, offset"""

    def __init__(self, t):
        self.key = t.untyped_storage().data_ptr()
        self.numel = t.untyped_storage().nbytes() // t.element_size()
        self.dtype, self.shape, self.stride, self.offset = t.dtype, tuple(t.shape), tuple(t.stride()), t.storage_offset()


def record(ops, fn):
    """[(op, {argument: Spec or value}, options the launch ran under)] of the wrapped ops calls that fn() makes"""
    calls, alive = [], []
    orig = {n: getattr(ops, n) for n in WRAPPED}
    sigs = {n: inspect.signature(f) for n, f in orig.items()}

    def wrap(n):
        def f(*a, **k):
            ba = sigs[n].bind(*a, **k)
            ba.apply_defaults()
            rec = {key: (Spec(v) if isinstance(v, torch.Tensor) else v) for key, v in ba.arguments.items()}
            if n == GNF:        # per-channel moments or a conv epilogue's channel quads?  (the entries behind a quad's first are zero)
                m = ba.arguments["moments"]
                rec["_quad"] = bool((m.reshape(m.shape[0], -1, 4, 2)[:, :, 1:] == 0).all())
            alive.extend(v for v in ba.arguments.values() if isinstance(v, torch.Tensor))   # (no storage is reused while named by address)
            out = orig[n](*a, **k)
            alive.append(out)
            rec["_tile"] = int(ops._lib.get_option("last_gemm_tile")) if n == CONV else None
            calls.append((n, rec))
            return out
        return f
    try:
        for n in WRAPPED:
            setattr(ops, n, wrap(n))
        keep = fn()
        torch.cuda.synchronize()
    finally:
        for n, f in orig.items():
            setattr(ops, n, f)
    del alive, keep
    return calls


def conv_from_record(a):
    """cp(...) of a recorded conv2d_nhwc call: the views' storage offsets join the descriptor's, the storages keep their sizes"""
    x, out, res = a["x"], a["out"], a["res"]
    B = x.shape[0] if a["B"] is None else a["B"]
    p = cp(a["Cin"], a["Cout"], a["KH"], a["KW"], a["stride"], a["pad"], a["H"], a["W"], B, act=a["act"], up=int(a["up"]), pad_w=a["pad_w"],
           out_w=a["out_w"], out_h=a["out_h"], out_row_pitch=a["out_row_pitch"], c_batch_stride=a["c_batch_stride"], ldc=a["ldc"],
           res_batch_stride=a["res_batch_stride"], ldr=a["ldr"], a_batch_stride=a["a_batch_stride"], a_offset=x.offset + a["a_offset"],
           x_numel=x.numel, bias=a["bias"] is not None, bias2=a["bias2"] is not None, w_group=a["w_group"],
           moments=None if a["moments"] is None else ("acc" if a["moments_accumulate"] else "plain"))
    p["c_offset"] = a["c_offset"] + (out.offset if out is not None else 0)
    if out is not None:
        p["out_numel"] = out.numel
    if res is not None:
        p["res"] = "alias" if (out is not None and res.key == out.key) else "sep"
        p["res_offset"], p["res_numel"] = res.offset + a["res_offset"], res.numel
    if a["bias2"] is not None:
        assert a["bias2"].stride == (a["Cout"], 1)
    return p


def replay(ops, calls, label, min256):
    """every recorded launch on fresh poisoned storages with its recorded geometry, under gemm_min256 = min256: the forms taken"""
    forms = []
    kappa = KAPPA.setdefault(label, {})
    for i, (op, a) in enumerate(calls):
        name = f"{label} #{i} {op} min256={min256}"
        with options(ops, gemm_min256=min256):
            if op == CONV:
                p = conv_from_record(a)
                for j, kind in enumerate(R.CONV_KINDS):
                    tile, _, _ = run_conv(ops, p, kind, 1000 * i + j, f"{name} {kind}")
                if min256 == 128:
                    assert tile == a["_tile"], (name, tile, a["_tile"])
                FORMS.setdefault((label, f"#{i} {p['KH']}x{p['KW']}s{p['stride']} {p['Cin']}>{p['Cout']} {p['H']}x{p['W']} B{p['B']}" +
                                  (f" up{p['up']}" if p["up"] else "")), {})[(1, 1, min256)] = tile
                forms.append(tile)
            elif op == NARROW:
                B, H, W, Cin = a["x"].shape
                ldy = a["ldy"] if a["out"] is None else a["out"].shape[-1]
                for j, kind in enumerate(R.CONV_KINDS):
                    run_narrow(ops, B, H, W, Cin, a["Cout"], ldy, kind, 1000 * i + j, f"{name} {kind}", bias=a["bias"] is not None)
            elif op == IMAGE:
                B, Cin, H, W = a["x_nchw"].shape
                for j, kind in enumerate(R.CONV_KINDS):
                    run_image(ops, B, Cin, H, W, a["w"].shape[0], kind, 1000 * i + j, f"{name} {kind}", a["moments"] is not None)
            elif op == STEM:
                B, H, W, _ = a["x_nhwc"].shape
                for j, kind in enumerate(R.CONV_KINDS):
                    run_stem(ops, B, H, W, a["Cout"], kind, 1000 * i + j, f"{name} {kind}")
            elif op == GNM:
                x = a["x"]
                B, C = x.shape[0], x.shape[-1]
                HW = math.prod(x.shape) // (B * C)
                for j, kind in enumerate(("random", "large_mean", "outlier")):
                    gen = torch.Generator(device=DEV).manual_seed(1000 * i + j)
                    xx, _ = R.gn_input(kind, B, HW, C, 1, gen, DEV)
                    mom = ops.groupnorm_moments(xx)
                    torch.cuda.synchronize()
                    want, bound = R.gn_moments_expect(xx)
                    note("groupnorm_moments", R.assert_entries(f"{name} {kind}", mom, want, bound))
            else:
                x = a["x"]
                B, C = x.shape[0], x.shape[-1]
                HW = math.prod(x.shape) // (B * C)
                form = "direct" if op == GN else ("quad" if a["_quad"] else "chan")
                pre = a["pre_add"] is not None
                for j, kind in enumerate(R.GN_KINDS):
                    if form == "quad" and pre:
                        raise AssertionError(f"{name}: channel-quad moments with a pre_add")
                    _, info, _ = run_gn(ops, B, HW, C, a["G"], kind, 1000 * i + j, f"{name} {kind}", act=a["act"], eps=a["eps"], pre=pre,
                                        post=a["post_add"] is not None, form=form, w_group=a["w_group"], key=f"replay groupnorm {form} {kind}", one_rounding=False)
                    kappa[kind] = max(kappa.get(kind, 0.0), info["kappa"])
    return forms


def _res_launches(first, shortcut):
    return [first, CONV, GNF] + ([CONV] if shortcut else []) + [CONV]


def vae_decode_expected(boc):
    """the launches of AutoencoderKL.decode (x2i_amd/vae.py; up_phases = 2, epilogue moments, narrow conv_out), in order"""
    rev = list(reversed(boc))
    want = [CONV] + _res_launches(GNF, False) + [GNF] + _res_launches(GN, False)        # conv_in, mid: resnet, attention's norm, resnet
    prev = rev[0]
    for i, co in enumerate(rev):
        for j in range(3):
            want += _res_launches(GNF, j == 0 and prev != co)
        if i != len(rev) - 1:
            want += [CONV] * 4
        prev = co
    return want + [GNF, NARROW]


def vae_encode_expected(boc):
    want = [IMAGE]
    prev = boc[0]
    for i, co in enumerate(boc):
        for j in range(2):
            want += _res_launches(GNF, j == 0 and prev != co)
        if i != len(boc) - 1:
            want += [CONV]
        prev = co
    return want + _res_launches(GNF, False) + [GNF] + _res_launches(GN, False) + [GNF, CONV]


CNX_PREPARE = [STEM, GN, CONV, GN, CONV, GN, GN, CONV, GNM]                              # embedding, down_res.0 norm1 + conv1, its moments
CNX_CHAINED = CNX_PREPARE + [GNF, CONV, CONV, GN, CONV, GN, CONV, CONV, CONV, CONV, GN, CONV, GN, CONV]
CNX_COMPOSED_TRUNK = [GNF, CONV, CONV, CONV, GN, CONV, GN, CONV, CONV, CONV, CONV, CONV, GN, CONV, GN]
CNX_TRAIN_FORWARD = CNX_CHAINED
CNX_TRAIN_BACKWARD = [CONV, CONV] + [CONV] * 4 + [CONV, CONV, CONV] + [CONV] * 4 + [CONV, CONV, CONV, CONV]

BOC = (128, 128, 256, 256)
_rec = {}


def recording(ops, which):
    if which in _rec:
        return _rec[which]
    from oracle import flux as OF
    from x2i_amd.lightcontrol import ControlNeXtBank, ControlNeXtModel
    from x2i_amd.lightcontrol_train import ControlNeXtTrainer
    from x2i_amd.vae import AutoencoderKL
    g = torch.Generator().manual_seed(7)
    if which.startswith("vae"):
        vae = AutoencoderKL(block_out_channels=BOC, device=DEV, with_encoder=which == "vae_encode").init_random_(seed=1)
        if which == "vae_decode":
            z = torch.randn((2, 16, 8, 12), generator=g).to(DEV)
            calls = record(ops, lambda: vae.decode(z, return_dict=False)[0])
            want = vae_decode_expected(BOC)
        else:
            img = torch.rand((2, 3, 64, 96), generator=g).to(DEV) * 2 - 1
            calls = record(ops, lambda: vae.encode(img, return_dict=False)[0].mode())
            want = vae_encode_expected(BOC)
    else:
        def net(seed):
            m = ControlNeXtModel(device=DEV)
            sd = OF.random_controlnext_state_dict(seed=seed)
            m.load_state_dict({k: v.to(torch.bfloat16) for k, v in sd.items()}, strict=True)
            return m
        hint = torch.rand((2, 3, 128, 128), generator=g).to(DEV, torch.bfloat16)
        t = torch.full((2,), 750.0, device=DEV)
        if which == "controlnext_chained":
            m = net(3)
            m.compose = False
            calls = record(ops, lambda: m.forward(hint, t)["out"])
            want = CNX_CHAINED
        elif which == "controlnext_bank":
            nets = [net(3 + i) for i in range(3)]
            assert ControlNeXtBank.eligible(nets)

            def run():
                bank = ControlNeXtBank(nets, hint)
                x, h, w = bank.trunk(ControlNeXtModel.timestep_features(bank.prep, t))
                return [n._final(x[i * 2:(i + 1) * 2], h, w) for i, n in enumerate(nets)]
            for n in nets:
                n._composed(64, 64)      # (the composed weights are made once per weight set, not per step: outside the recording)
            calls = record(ops, run)
            want = (CNX_PREPARE + [CONV]) * 3 + CNX_COMPOSED_TRUNK + [CONV] * 3
        else:
            tr = ControlNeXtTrainer([net(3)])

            def run():
                outs = tr.forward(hint, t)
                tr.backward([torch.randn(o.shape, device=DEV).to(torch.bfloat16) for o in outs])
                return outs
            calls = record(ops, run)
            want = CNX_TRAIN_FORWARD + CNX_TRAIN_BACKWARD
    names = [c[0] for c in calls]
    assert names == want, (which, names)
    _rec.clear()
    _rec[which] = calls
    return calls


RECORDINGS = ["vae_decode", "vae_encode", "controlnext_chained", "controlnext_bank", "controlnext_train"]


@pytest.mark.parametrize("min256", [128, 1], ids=["model_thresholds", "min256_1"])
@pytest.mark.parametrize("which", RECORDINGS)
def test_model_conv_and_groupnorm_launches_vs_fp64(ops, which, min256):
    t0 = time.time()
    calls = recording(ops, which)
    forms = replay(ops, calls, which, min256)
    print(f"\n  {which}: {len(calls)} launches replayed under gemm_min256 = {min256}; conv forms: " +
          ", ".join(f"{f} x {forms.count(f)}" for f in sorted(set(forms))) + "; largest kappa per operand kind: " +
          ", ".join(f"{k} {v:.4g}" for k, v in KAPPA[which].items()))
    print_worst(f"{which} min256={min256}", t0)


# ---------------------------------------------------------------------------------------------------------------- (e) negative controls
def _rejected(fn, *needles):
    with pytest.raises(AssertionError) as e:
        fn()
    msg = str(e.value)
    for n in needles:
        assert n in msg, (n, msg)
    return msg


def test_negative_controls_on_real_kernel_output(ops):
    """a real kernel output against a deliberately wrong expectation: rejected, and the message names the sample, pixel and channel"""
    # pad_w off by one.  The input is constant along W, so a filter shifted by one column sees the same values everywhere but where the padding
    # comes in: the wrong expectation differs at the border columns only.  A window of a larger input and an interleaved output
    # (ldc = 2 Cout): the checker's strided views on device tensors
    p = cp(128, 256, 3, 3, 1, 1, 32, 40, 2, ldc=512, c_offset=256, c_batch_stride=32 * 40 * 512, a_offset=640, x_numel=2 * 32 * 40 * 128 + 1024, act=RELU, bias2=True)
    with options(ops, gemm_min256=1):
        st = conv_state(p, "random", 41)
        for z in range(p["B"]):
            v = R.item_view(st.x, geom(p), z, p["a_offset"], None)
            v.copy_(v[:, :1, :].expand(-1, p["W"], -1).clone())
        assert conv_launch(ops, p, st) == 5256
    conv_check_output(p, st, "negative control, right expectation")
    wrong = dict(p, pad_w=0, out_w=40)
    msg = _rejected(lambda: conv_check_output(wrong, st, "pad_w off by one"), "pad_w off by one", "sample 0", "output pixel (oy=", "channel ")
    ox = int(msg.split("ox=")[1].split(")")[0])
    assert ox in (0, 39), msg                       # a border column (left: a padded tap taken for real; right: a real tap taken for padding)
    print("\n  " + msg)

    # bias2 behind the ReLU instead of in front of it
    def bias2_behind_relu():
        g = geom(p)
        rep = R.Report("bias2 behind the ReLU")
        out4 = st.out.as_strided(*out_view(p))
        for z in range(p["B"]):
            A = R.gather(R.item_view(st.x, g, z, p["a_offset"], None), g, 0, g.M)
            want, bound, d = R.gemm_expect(A, st.w, st.bias, act=RELU)
            want = want + st.bias2[z].double()
            rep.check(out4[z].reshape(g.M, -1), want, R._round_bound(want, d, False), d, item=z, where=R.where_pixel(g.OW, z))
        rep.done()
    msg = _rejected(bias2_behind_relu, "bias2 behind the ReLU", "sample 0", "output pixel (oy=", "channel ")
    print("  " + msg)

    # GroupNorm: eps 1e-5 where the kernel was given 1e-6, on the `const` kind (a constant group's r = 1 / sqrt(eps); a nearly constant
    # group's variance is of the order of eps, so its two off-constant elements move by a large factor)
    B, HW, C, G = 2, 257, 128, 32
    gen = torch.Generator(device=DEV).manual_seed(43)
    x, _ = R.gn_input("const", B, HW, C, G, gen, DEV)
    w, b = R.gn_affine(C, gen, DEV)
    y = ops.groupnorm_nhwc(x, w, b, G, 1e-6)
    torch.cuda.synchronize()
    rep = R.Report("gn right eps")
    R.check_groupnorm(rep, x, y, w, b, G, 1e-6)
    rep.done()

    def wrong_eps():
        rep = R.Report("gn eps 1e-5 for 1e-6")
        R.check_groupnorm(rep, x, y, w, b, G, 1e-5)
        rep.done()
    msg = _rejected(wrong_eps, "gn eps 1e-5 for 1e-6", "sample 0", "pixel ", "channel ", "group ")
    grp = int(msg.split("group ")[1].split(" ")[0].rstrip(":,"))
    assert grp % 3 == 1, msg                        # a nearly constant group: two elements one ulp off the constant
    print("  " + msg)


def test_print_worst():
    """(last: the tables of worst shares and of kernel forms over everything this module ran)"""
    print_worst("all", time.time())
    print("  kernel forms, {(conv_w4, conv_korder, gemm_min256): last_gemm_tile}:")
    for (group, label), row in FORMS.items():
        print(f"    {group}: {label}: {row}")
    print("  largest kappa met in the recordings' GroupNorm replays, per operand kind:")
    for which, row in KAPPA.items():
        print(f"    {which}: " + ", ".join(f"{k} {v:.4g}" for k, v in row.items()))
