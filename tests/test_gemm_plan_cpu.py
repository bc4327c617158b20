"""The GEMM launcher's decisions without a GPU: csrc/gemm.hip runs checks -> plan -> launch, and x2i_gemm_plan_describe (csrc/x2i_kernels.h, bound
here, not part of the C ABI) runs the first two on made-up, never dereferenced addresses for cus = 256 compute units.

* The model's launches: the ten launches of a denoise step (x2i_amd/flux.py: D = 3072, H = 24, St = 512) in the four configurations and seven
  option variants of tests/test_gemm_fp64_gpu.py, against that module's DEFAULT_FORMS / ALT_FORMS -- tables measured on an MI355X.
* The forms other GPU tests assert (test_gemm_w4_gpu, test_conv_w4_gpu, test_fp8_gpu), one row each, and every (shape, option, epilogue) of the
  e4m3 table of tests/test_fp8_fp64_gpu.py with that module's geometry.
* Batch independence of the two kinds of kernel that sum in another order than the rest -- the FX split and the persistent convolution
  kernels: whether they are chosen is the same for every batch 1..8, over a grid of shapes.
* Plan sanity on every row, and the refusals' codes and messages stage by stage."""
import ctypes as C
import itertools

import pytest

from tests.test_conv_w4_gpu import CASES, CASES128
from tests.test_fp8_fp64_gpu import A_ROWS as FP8_A_ROWS, EPILOGUES as FP8_EPILOGUES, GEMM_ROWS as FP8_ROWS, gemm_n as fp8_n
from tests.test_gemm_fp64_gpu import ALT_FORMS, CONFIGS, DEFAULT_FORMS, LAUNCHES, ST
from x2i_amd import _lib
from x2i_amd._lib import ACT_GELU_TANH, ConvDesc, Fp8Desc, GemmArgs, QkvDesc

CUS = 256
D, H = 3072, 24
PER_LAUNCH = ("grid_x", "grid_y", "grid_z", "threads", "lds", "M", "tilesM", "tilesN", "gm", "nbatch", "sk_on", "fx_v0")
DESCRIBE_LEN = 2 + 2 * len(PER_LAUNCH) + 1        # csrc/x2i_kernels.h: X2I_PLAN_DESCRIBE_LEN
SMEM2_BYTES, SMEM2P_BYTES, SMEM5C_BYTES = 8 * 18432, 160 * 1024, 160 * 1024       # csrc/gemm_device.h
LDS_SIZES = {0, 64 * 1024, SMEM2_BYTES, SMEM2P_BYTES, SMEM5C_BYTES}
FX, CONV_PERSISTENT = 3256, (5256, 5512)
ROWS = [0]                                        # rows described so far (printed by the last test)


@pytest.fixture(scope="module")
def lib():
    lib = _lib.load()
    fn = lib.x2i_gemm_plan_describe
    fn.argtypes = [C.POINTER(GemmArgs), C.POINTER(ConvDesc), C.POINTER(QkvDesc), C.POINTER(Fp8Desc), C.POINTER(GemmArgs), C.POINTER(QkvDesc),
                   C.c_int, C.POINTER(C.c_int64)]
    fn.restype = C.c_int
    return lib


@pytest.fixture
def opt(lib):
    saved = {}

    def set_(name, value):
        saved.setdefault(name, _lib.set_option(name, value))
    yield set_
    for k, v in saved.items():
        _lib.set_option(k, v)


_next = [1 << 40]


def ptr(nbytes=1 << 32):
    """a made-up device address, 256-byte aligned, `nbytes` away from the next one"""
    p = _next[0]
    _next[0] += (nbytes + 255) // 256 * 256
    return p


def workspace(a, lib, misalign=0):
    a.workspace, a.workspace_bytes = ptr() + misalign, lib.x2i_streamk_workspace_bytes()
    return a


def gemm(lib, M, N, K, batch=1, a_bs=0, lda=None, c_bs=0, ldc=None, act=0, gated=False, a_off=0, c_off=0, ws=True):
    """x2i_gemm_args as ops.gemm fills them (bf16, W [N, K] contiguous); gated: the in-place gated residual of the model (res = C)"""
    a = GemmArgs(A=ptr() + 2 * a_off, a_batch_stride=a_bs, lda=lda or K, W=ptr(), ldw=K, bias=ptr(), C=ptr() + 2 * c_off, c_batch_stride=c_bs,
                 ldc=ldc or N, M=M, N=N, K=K, batch=batch, act=act)
    if gated:
        a.res, a.res_batch_stride, a.ldr, a.gate, a.gate_batch_stride = a.C, c_bs, a.ldc, ptr(), N
    return workspace(a, lib) if ws else a


def qkv_desc(S, tok_off, rows):
    Spad = (S + 127) // 128 * 128
    return QkvDesc(norm_q=ptr(), norm_k=ptr(), cos=ptr(), sin=None, Q=ptr(), K=ptr(), VT=ptr(), H=H, Spad=Spad, tok_off=tok_off, rows_per_sample=rows,
                   eps=1e-6, q_scale=0.1275, vt_perm=0)


def conv(Cin, Cout, KH, KW, s, p, Hh, Ww, B, res=False):
    """x2i_gemm_args + x2i_conv_desc as ops.conv2d_nhwc fills them (dense NHWC in and out, no workspace)"""
    OH, OW = (Hh + 2 * p - KH) // s + 1, (Ww + 2 * p - KW) // s + 1
    a = GemmArgs(A=ptr(), a_batch_stride=Hh * Ww * Cin, lda=Cin, W=ptr(), ldw=KH * KW * Cin, bias=ptr(), C=ptr(), c_batch_stride=OH * OW * Cout, ldc=Cout,
                 res=ptr() if res else None, res_batch_stride=OH * OW * Cout, ldr=Cout, M=OH * OW, N=Cout, K=KH * KW * Cin, batch=B)
    return a, ConvDesc(H=Hh, W=Ww, Cin=Cin, KH=KH, KW=KW, stride=s, pad=p)


def describe(lib, a, cd=None, qd=None, f=None, a1=None, q1=None, cus=CUS):
    """-> (code, plan dict) or (code, message)"""
    out = (C.c_int64 * DESCRIBE_LEN)(*([-7] * DESCRIBE_LEN))
    ref = lambda x: C.byref(x) if x is not None else None
    rc = lib.x2i_gemm_plan_describe(ref(a), ref(cd), ref(qd), ref(f), ref(a1), ref(q1), cus, out)
    if rc:
        return rc, lib.x2i_last_error().decode()
    v = list(out)
    n = len(PER_LAUNCH)
    of = a1 if a1 is not None and v[0] not in (2256, FX) else a          # (a pair that is not grouped: the second launch's plan)
    plan = dict(form=v[0], launches=[dict(zip(PER_LAUNCH, v[2 + i * n:2 + (i + 1) * n])) for i in range(v[1])], chunk=v[-1], M=of.M, batch=of.batch)
    ROWS[0] += 1
    check_plan(plan, cus)
    return rc, plan


def check_plan(plan, cus):
    ls = plan["launches"]
    assert len(ls) == (2 if plan["form"] == 1256 else 1), plan
    for l in ls:
        assert l["lds"] in LDS_SIZES and l["grid_x"] >= 1 and l["grid_y"] >= 1 and l["grid_z"] >= 1, plan
        if l["lds"] == SMEM2P_BYTES:        # the persistent kernels (and only they) take all 160 KiB: at most one workgroup per CU
            assert l["grid_x"] <= cus and l["grid_y"] == l["grid_z"] == 1 and l["threads"] == 256, plan
    if len(ls) == 2:                        # a peeled tail: whole 256-row tiles in front, the other rows behind, together M
        main, tail = ls
        assert main["M"] == main["tilesM"] * 256 and main["M"] + tail["M"] == plan["M"] and tail["tilesM"] == (tail["M"] + 127) // 128, plan
        assert main["sk_on"] == 0 and tail["lds"] == 64 * 1024, plan
    elif plan["form"] != 2256 and plan["form"] != 0:
        assert ls[0]["M"] == plan["M"], plan
    if plan["form"] == FX:
        assert ls[0]["grid_x"] == cus and 1 <= ls[0]["fx_v0"] <= cus // 8, plan
    if plan["form"] in CONV_PERSISTENT:
        assert 1 <= plan["chunk"] <= plan["batch"] and ls[0]["nbatch"] == plan["chunk"], plan
    else:
        assert plan["chunk"] == 0, plan


def form_of(lib, *args, **kw):
    rc, plan = describe(lib, *args, **kw)
    assert rc == 0, plan
    return plan["form"]


# ---------------------------------------------------------------------------------------------------------------- the model's launches
def model_launches(lib, B, side):
    """name -> describe arguments of the ten GEMM launches of FluxTransformer2DModel.prepare_conditioning + denoise (x2i_amd/flux.py)"""
    Si = (side // 16) ** 2
    S = ST + Si
    img = dict(batch=B, a_bs=S * D, lda=D, a_off=ST * D)      # the image rows of a [B, S, D] buffer; the text rows: without the offset
    txt = dict(batch=B, a_bs=S * D, lda=D)
    x_img, x_txt = dict(c_bs=S * D, ldc=D, c_off=ST * D, gated=True), dict(c_bs=S * D, ldc=D, gated=True)    # X += gate * linear, in place

    def pair(g0, g1):
        return dict(a=g0, a1=g1)
    return {
        "context_embedder": dict(a=gemm(lib, B * ST, D, 4096)),
        "x_embedder": dict(a=gemm(lib, Si, D, 64, batch=B, a_bs=Si * 64, lda=64, c_bs=S * D, ldc=D, c_off=ST * D)),
        "qkv_pair": dict(a=gemm(lib, Si, 3 * D, D, **img), qd=qkv_desc(S, ST, Si), a1=gemm(lib, ST, 3 * D, D, **txt), q1=qkv_desc(S, 0, ST)),
        "to_out_pair": pair(gemm(lib, Si, D, D, **img, **x_img), gemm(lib, ST, D, D, **txt, **x_txt)),
        "ff0_pair": pair(gemm(lib, Si, 4 * D, D, **img, c_bs=Si * 4 * D, ldc=4 * D, c_off=B * ST * 4 * D, act=ACT_GELU_TANH),
                         gemm(lib, ST, 4 * D, D, **txt, c_bs=ST * 4 * D, ldc=4 * D, act=ACT_GELU_TANH)),
        "ff2_pair": pair(gemm(lib, Si, D, 4 * D, batch=B, a_bs=Si * 4 * D, lda=4 * D, a_off=B * ST * 4 * D, **x_img),
                         gemm(lib, ST, D, 4 * D, batch=B, a_bs=ST * 4 * D, lda=4 * D, **x_txt)),
        "single_qkv": dict(a=gemm(lib, B * S, 3 * D, D), qd=qkv_desc(S, 0, S)),
        "proj_mlp": dict(a=gemm(lib, B * S, 4 * D, D, ldc=5 * D, c_off=D, act=ACT_GELU_TANH)),
        "single_proj_out": dict(a=gemm(lib, S, D, 5 * D, batch=B, a_bs=S * 5 * D, lda=5 * D, c_bs=S * D, ldc=D, gated=True)),
        "final_proj_out": dict(a=gemm(lib, B * Si, 64, D)),
    }


MODEL_CASES = [(cfg, None, None, DEFAULT_FORMS[cfg]) for cfg in CONFIGS] + ALT_FORMS


@pytest.mark.parametrize("cfg,name,value,want", MODEL_CASES, ids=[f"{c}-{n}={v}" if n else c for c, n, v, _ in MODEL_CASES])
def test_model_launch_forms_match_the_measured_tables(lib, opt, cfg, name, value, want):
    if name:
        opt(name, value)
    launches = model_launches(lib, *CONFIGS[cfg])
    assert list(launches) == LAUNCHES
    got = {n: form_of(lib, **kw) for n, kw in launches.items()}
    assert got == want


# ---------------------------------------------------------------------------------------------------------------- forms the GPU tests assert
def test_forms_asserted_by_the_gpu_tests(lib, opt):
    M, N, K = 4 * 4608, 3072, 3072
    # tests/test_gemm_w4_gpu.py: stream-K on a workspace, the peeled tail without one
    assert form_of(lib, gemm(lib, M, N, K)) == 256 and form_of(lib, gemm(lib, M, N, K, ws=False)) == 1256
    rc, plan = describe(lib, gemm(lib, M, N, K))
    assert plan["launches"][0]["sk_on"] == 1 and plan["launches"][0]["grid_x"] == CUS

    def proj_out(S, B, **kw):
        return gemm(lib, S, 3072, 15360, batch=B, a_bs=S * 15360, c_bs=S * 3072, gated=True, **kw)
    # ... FX by default for a 512^2 sample's proj_out at any batch, whole tiles for a 1024^2 sample's
    assert form_of(lib, proj_out(1536, 1)) == FX and form_of(lib, proj_out(1536, 3)) == FX and form_of(lib, proj_out(4608, 1)) != FX
    opt("gemm_fx", 1)
    assert form_of(lib, proj_out(4608, 1)) == FX and form_of(lib, proj_out(4608, 3)) == FX
    assert form_of(lib, proj_out(4608, 1, ws=False)) != FX
    opt("gemm_fx", 2)
    # tests/test_fp8_gpu.py: e4m3 operands (one byte per element of A and W)
    f = Fp8Desc(a_scale=ptr(), a_scale_batch_stride=0, w_scale=ptr(), alpha=1.0, out_fp8=0, out_inv_scale=1.0)
    assert form_of(lib, gemm(lib, M, N, K), f=f) == 9256
    opt("gemm_streamk", 0)
    assert form_of(lib, gemm(lib, M, N, K), f=f) == 8256
    opt("gemm_streamk", 1)
    opt("gemm_fp8_persist", 0)
    assert form_of(lib, gemm(lib, M, N, K), f=f) == 7256


@pytest.mark.parametrize("row", list(FP8_ROWS))
def test_e4m3_forms_asserted_by_the_fp64_gpu_tests(lib, opt, row):
    """tests/test_fp8_fp64_gpu.py: one describe per (shape, option, epilogue) of its GEMM table, with that module's geometry (A rows behind an
    offset in a [batch, 428, K] buffer, C at an offset into rows of ldc = N + 16), and its fused-QKV launches"""
    M, N0, K, batch, name, value, want, _ = FP8_ROWS[row]
    if name:
        opt(name, value)
    for epi, (scaled, act, out8, oinv, alpha, gated) in FP8_EPILOGUES.items():
        N = fp8_n(N0, out8)
        ldc = N + 16
        c_bs = M * ldc + 64 if batch > 1 else 0
        kw = dict(batch=batch, a_bs=FP8_A_ROWS * K, lda=K) if batch > 1 else {}
        a = gemm(lib, M, N, K, c_bs=c_bs, ldc=ldc, act=act, gated=gated, **kw)
        f = Fp8Desc(a_scale=ptr() if scaled else None, a_scale_batch_stride=M if batch > 1 else 0, w_scale=ptr() if scaled else None, alpha=alpha,
                    out_fp8=int(out8), out_inv_scale=oinv)
        assert form_of(lib, a, f=f) == want, (row, epi)


@pytest.mark.parametrize("M,Hq,K,batch,want", [(300, 2, 256, 2, 7256), (300, 2, 384, 2, 8256), (2 * FP8_A_ROWS, 2, 256, 1, 7256),
                                               (2 * FP8_A_ROWS, 2, 384, 1, 8256), (8000, 8, 2048, 1, 9256)])
def test_e4m3_qkv_forms_asserted_by_the_fp64_gpu_tests(lib, M, Hq, K, batch, want):
    S = M if M == 8000 else FP8_A_ROWS
    qd = qkv_desc(S, FP8_A_ROWS - 300 if batch > 1 else 0, 300 if batch > 1 else S)
    qd.H = Hq
    f = Fp8Desc(a_scale=ptr(), a_scale_batch_stride=M if batch > 1 else 0, w_scale=ptr(), alpha=1.0, out_fp8=0, out_inv_scale=1.0)
    kw = dict(batch=batch, a_bs=FP8_A_ROWS * K, lda=K) if batch > 1 else {}
    assert form_of(lib, gemm(lib, M, 3 * Hq * 128, K, **kw), qd=qd, f=f) == want


@pytest.mark.parametrize("case,new,old", [(c, 5256, 256) for c in CASES] + [(c, 5512, 128) for c in CASES128])
def test_conv_forms_asserted_by_the_gpu_tests(lib, opt, case, new, old):
    """tests/test_conv_w4_gpu.py::_both: gemm_min256 = 1; conv_w4 = 1 -> the persistent kernels, 0 -> the older ones; with and without a residual"""
    opt("gemm_min256", 1)
    for res in (False, True):
        for korder in (0, 1):
            opt("conv_korder", korder)
            assert form_of(lib, *conv(*case, res=res)) == new
        opt("conv_w4", 0)
        assert form_of(lib, *conv(*case, res=res)) == old
        opt("conv_w4", 1)


# ---------------------------------------------------------------------------------------------------------------- batch independence
BATCHES = range(1, 9)


def test_fx_choice_depends_on_the_batch_item_only(lib):
    """FX sums along K in another order than whole tiles: "form == 3256" must be one answer for every batch a sample may ride in."""
    taken = 0
    grid = itertools.product((512, 1024, 1536, 3969, 4096, 4608), (3072, 9216, 12288), (3072, 12288, 15360), ("plain", "gelu", "gated"), (True, False))
    for M, N, K, epi, ws in grid:
        fx = {form_of(lib, gemm(lib, M, N, K, batch=b, a_bs=M * K, c_bs=M * N, act=ACT_GELU_TANH if epi == "gelu" else 0, gated=epi == "gated",
                                ws=ws)) == FX for b in BATCHES}
        assert len(fx) == 1, (M, N, K, epi, ws)
        taken += fx.pop()
    assert 0 < taken < 6 * 3 * 3 * 3 * 2          # (the grid holds both answers)


@pytest.mark.parametrize("min256", [128, 1])
def test_persistent_conv_choice_depends_on_the_batch_item_only(lib, opt, min256):
    """The persistent convolution kernels run the product K order: "form in {5256, 5512}" must be one answer for every batch.  (min256 = 128 is the
    default: 1024^2-sized items only; 1 is what the GPU tests set to reach these kernels with small images)"""
    opt("gemm_min256", min256)
    taken = 0
    for HW, Cin, Cout in itertools.product((32, 64, 128), (128, 256, 512), (128, 256, 512)):
        pers = {form_of(lib, *conv(Cin, Cout, 3, 3, 1, 1, HW, HW, b)) in CONV_PERSISTENT for b in BATCHES}
        assert len(pers) == 1, (HW, Cin, Cout)
        taken += pers.pop()
    assert 0 < taken < 27


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_keep_their_codes_and_messages(lib):
    """One case or more per stage: code and message, in the launcher's order of refusal"""
    ARG, SHAPE, ALIGN = -1, -2, -3
    f = Fp8Desc(a_scale=ptr(), a_scale_batch_stride=0, w_scale=ptr(), alpha=1.0, out_fp8=0, out_inv_scale=1.0)
    a = gemm(lib, 512, 512, 512)
    a.A = None
    assert describe(lib, a) == (ARG, "gemm: null pointer")
    assert describe(lib, a, f=f) == (ARG, "gemm_fp8: null pointer")
    a = gemm(lib, 512, 512, 512)
    a.gate = ptr()
    assert describe(lib, a) == (ARG, "gemm: gate without residual")
    a = gemm(lib, 512, 512, 512, batch=0)
    assert describe(lib, a) == (SHAPE, "gemm: bad shape M=512 N=512 K=512 batch=0")
    # convolution descriptor
    a, cd = conv(96, 256, 3, 3, 1, 1, 32, 32, 1)
    assert describe(lib, a, cd) == (SHAPE, "conv: Cin must be a multiple of 64 (Cin=96)")
    a, cd = conv(128, 256, 3, 3, 1, 1, 32, 32, 1)
    a.M += 1
    assert describe(lib, a, cd) == (SHAPE, "conv: M=1025 K=1152 do not match OH*OW=1024, KH*KW*Cin=1152")
    a, cd = conv(128, 256, 3, 3, 1, 1, 32, 32, 1)
    cd.moments = ptr()
    assert describe(lib, a, cd) == (ARG, "conv: moments without moments_scratch (x2i_conv_moments_scratch_floats)")
    # fused QKV descriptor
    a, qd = gemm(lib, 4608, 9000, 3072), qkv_desc(4608, 0, 4608)
    assert describe(lib, a, qd=qd) == (SHAPE, "gemm_qkv: N=9000 must be 3*H*128 (H=24)")
    a = gemm(lib, 4608, 9216, 3072)
    qd.Q += 8
    assert describe(lib, a, qd=qd) == (ALIGN, "gemm_qkv: descriptor pointers must be 16-byte aligned")
    # pair
    assert describe(lib, gemm(lib, 512, 512, 512), a1=gemm(lib, 512, 512, 512), q1=qkv_desc(512, 0, 512)) == (ARG, "gemm_pair: null pointer / mixed kinds")
    # e4m3 operands
    assert describe(lib, gemm(lib, 4608, 3072, 3136), f=f) == (
        ALIGN, "gemm_fp8: needs K % 128 == 0 (K=3136), lda / ldw / a_batch_stride % 16 == 0, 16-byte aligned A / W")
    a = gemm(lib, 4608, 3072, 3072)
    a.out_f32 = 1
    assert describe(lib, a, f=f) == (ARG, "gemm_fp8: C2 / f32 output / per-batch W are not supported")
    # plan stage: the caller's workspace, where a launch would use it (stream-K; FX; e4m3 stream-K) and only there
    need = lib.x2i_streamk_workspace_bytes()
    msg = f"gemm: stream-K workspace must be 256-byte aligned and >= x2i_streamk_workspace_bytes() = {need} bytes (got {need})"
    bad = lambda a: workspace(a, lib, misalign=64)
    assert describe(lib, bad(gemm(lib, 4 * 4608, 3072, 3072))) == (ARG, msg)
    assert describe(lib, bad(gemm(lib, 1536, 3072, 15360, gated=True))) == (ARG, msg)
    assert describe(lib, bad(gemm(lib, 4 * 4608, 3072, 3072)), f=f) == (ARG, msg)
    assert describe(lib, bad(gemm(lib, 512, 3072, 3072)))[0] == 0
    # plan stage: no kernel serves the problem
    assert describe(lib, gemm(lib, 4608, 3072, 3080)) == (
        SHAPE, "gemm: M=4608 N=3072 K=3080 batch=1 has no MFMA path (needs K %% 64 == 0, lda/ldw %% 8 == 0, 16-byte aligned A/W, operands below 2 GB) "
               "and is too large for the generic kernel")
    assert form_of(lib, gemm(lib, 100, 100, 100)) == 0
    a, cd = conv(128, 256, 3, 3, 1, 1, 32, 32, 1)
    a.A += 8
    assert describe(lib, a, cd) == (SHAPE, "conv: unsupported epilogue/alignment combination")
    a, qd = gemm(lib, 4608, 9216, 3072, lda=3076), qkv_desc(4608, 0, 4608)
    assert describe(lib, a, qd=qd) == (SHAPE, "gemm_qkv: the fused epilogue needs K % 64 == 0 (K=3072), lda/ldw % 8 == 0 (lda=3076 ldw=3072), 16-byte aligned "
                                              "A/W and operands below 2 GB")
    print(f"\n  {ROWS[0]} launches described so far in this module")
