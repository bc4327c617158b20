"""What x2i_amd/ops.py hands to the C ABI, as a recorded trace (no GPU, no libx2i_hip.so).

Every public wrapper of ops.py runs on small CPU tensors against a stub of the library that stores (export name, arguments) instead of
launching; a struct argument is stored as a dict of its fields, a pointer as [name of the test tensor it points into, byte offset]
("ret": the wrapper's return value, "internal": any other buffer, None: null), a float by repr.  The trace must equal tests/abi_trace.json
case by case: a field that a wrapper stops setting, sets from another argument or offsets in other units shows up here, where on the GPU it
would only change what a kernel reads.  The file also pins the public names of ops and the signature of every public callable.

    python tests/test_ops_abi_cpu.py --record      rewrites tests/abi_trace.json from the ops.py of the working tree
"""
import ctypes as C
import importlib.util
import inspect
import json
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
TRACE = os.path.join(ROOT, "tests", "abi_trace.json")
BF16, F32, FP8, U8, I64 = torch.bfloat16, torch.float32, torch.float8_e4m3fn, torch.uint8, torch.int64
QUERY_SIZES = (96, 40, 160)   # what the stub's *_floats queries answer, call after call per export: a growing scratch shows as 96, 96, 160
WS_BYTES = 8192               # ... and x2i_streamk_workspace_bytes


def fresh_ops(path=None):
    """A private instance of ops.py (its caches start empty, the imported one keeps its own), bound to the package's one _lib."""
    from x2i_amd import _lib  # noqa: F401
    path = os.path.join(ROOT, "x2i_amd", "ops.py") if path is None else path
    spec = importlib.util.spec_from_file_location("x2i_amd._ops_abi_trace", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Recorder:
    """Stands in for the loaded library: every attribute is an export that stores its arguments and returns 0."""

    def __init__(self, signatures):
        self.signatures, self.calls, self.asked = signatures, [], {}

    def __getattr__(self, name):
        if not name.startswith("x2i_"):
            raise AttributeError(name)

        def export(*args):
            argtypes = self.signatures.get(name)
            assert argtypes is None or len(argtypes) == len(args), (name, len(args))
            self.calls.append((name, [self.raw(a, t) for a, t in zip(args, argtypes or [C.c_int32] * len(args))]))
            if name.endswith(("_floats", "_bytes")):
                k = self.asked[name] = self.asked.get(name, -1) + 1
                size = WS_BYTES if name.endswith("_bytes") else QUERY_SIZES[k % len(QUERY_SIZES)]
                if argtypes and argtypes[-1] == C.POINTER(C.c_int64):
                    args[-1]._obj.value = size
                    return 0
                return size
            return {"x2i_abi_version": 5, "x2i_last_error": b""}.get(name, 0)

        export.__name__ = name
        return export

    @staticmethod
    def raw(a, t):
        """the argument as the library would read it, pointers still as addresses: ("p", address) / ("s", {field: ...}) / plain values"""
        if t == C.c_void_p:
            v = a.value if isinstance(a, C.c_void_p) else a
            return ("p", int(v) if v else 0)
        if t == C.c_char_p:
            return a.decode()
        if t == C.c_float:
            return repr(float(a))
        if t in (C.c_int32, C.c_int64):
            return int(a)
        obj = a._obj   # byref(...)
        if isinstance(obj, C.Structure):
            assert isinstance(obj, t._type_), (type(obj), t._type_)
            d = {}
            for f, ft in obj._fields_:
                v = getattr(obj, f)
                d[f] = ("p", int(v) if v else 0) if ft == C.c_void_p else repr(v) if ft == C.c_float else int(v)
            return ("s", d)
        return "int64*"


class Case:
    """The tensors of one case, by name, and the wrapper calls made on them."""

    def __init__(self, ops, rec):
        self.ops, self.rec, self.tensors, self.out = ops, rec, {}, []

    def t(self, name, *shape, dtype=BF16):
        assert name not in self.tensors and name not in ("ret", "internal")
        x = torch.zeros(shape, dtype=U8 if dtype == FP8 else dtype)
        self.tensors[name] = x = x.view(FP8) if dtype == FP8 else x
        return x

    def where(self, addr, ret):
        if not addr:
            return None
        named = list(self.tensors.items()) + [("ret" if len(ret) == 1 else "ret%d" % i, r) for i, r in enumerate(ret)]
        for name, x in named:
            base = x.untyped_storage().data_ptr()
            if base <= addr < base + max(x.untyped_storage().nbytes(), 1):
                return [name, addr - base]
        return "internal"

    def norm(self, v, ret):
        if isinstance(v, tuple) and v[0] == "p":
            return self.where(v[1], ret)
        if isinstance(v, tuple) and v[0] == "s":
            return {f: self.norm(x, ret) for f, x in v[1].items()}
        return v

    def call(self, fn, *args, **kw):
        """fn(*args, **kw), a public callable of ops or its name: its library calls and what it returns join the case's trace"""
        fn = getattr(self.ops, fn) if isinstance(fn, str) else fn
        start = len(self.rec.calls)
        got = fn(*args, **kw)
        ret = [r for r in (got if isinstance(got, tuple) else (got,)) if isinstance(r, torch.Tensor)]
        shown = [self.where(r.data_ptr(), []) or "null" for r in ret]
        desc = [{"is": s if s != "internal" else "new", "shape": list(r.shape), "stride": list(r.stride()), "dtype": str(r.dtype)}
                for s, r in zip(shown, ret)]
        if not ret and got is not None:
            desc = got if isinstance(got, (bool, int, float, str)) else type(got).__name__
        self.out.append({"fn": fn.__name__, "calls": [[n, [self.norm(a, ret) for a in args_]] for n, args_ in self.rec.calls[start:]],
                         "ret": desc})
        return got


class FakeWorkspace:
    def __init__(self, case):
        self.buf, self.nbytes = case.t("ws", 256, dtype=U8), 256


# ------------------------------------------------------------------------------------------------------------------------ the cases
# name -> (function(case, ops), workspace: None / "fake"); a case named after a wrapper covers it, "name/variant" too
CASES = {}


def case(name, ws=None):
    def deco(fn):
        CASES[name] = (fn, ws)
        return fn
    return deco


def _gemm_full(c, tag="", out_f32=True):
    """every keyword of gemm() at a distinct non-default value"""
    o = c.ops
    W = c.t("Wbig" + tag, 2, 8, 12)[:, :, :10]     # [groups, N, K] of row stride 12
    return dict(A=c.t("A" + tag, 200), W=W, bias=c.t("bias" + tag, 2, 8), out=c.t("out" + tag, 300, dtype=F32 if out_f32 else BF16),
                M=5, batch=4, a_batch_stride=40, lda=14, c_batch_stride=60, ldc=18, act=o.ACT_SILU, gate=c.t("gate" + tag, 4, 8),
                gate_batch_stride=8, res=c.t("res" + tag, 300), res_batch_stride=62, ldr=19, out2=c.t("out2" + tag, 300),
                act2=o.ACT_GELU_TANH, out_f32=out_f32, a_offset=3, c_offset=7, res_offset=11, N=6, K=9, bias2=c.t("bias2" + tag, 4, 8),
                bias2_batch_stride=13, w_batch_stride=96, w_group=2)


@case("gemm")
@case("gemm/ws", ws="fake")
def _(c, o):
    c.call("gemm", c.t("A", 6, 16), c.t("W", 24, 16))
    c.call("gemm", c.t("A3", 2, 3, 16), c.tensors["W"], c.t("bias", 24))


@case("gemm/full", ws="fake")
@case("gemm/full_no_ws")
def _(c, o):
    c.call("gemm", **_gemm_full(c))
    c.call("gemm", **_gemm_full(c, "b", out_f32=False))


@case("gemm/alloc", ws="fake")
def _(c, o):
    A, W = c.t("A", 3, 5, 16), c.t("W", 24, 16)
    c.call("gemm", A, W, batch=3, M=5, a_batch_stride=80)
    c.call("gemm", A, W, out_f32=True, c_offset=2, res=c.t("res", 15, 24), act=o.ACT_GELU_ERF)
    c.call("gemm", A, W, batch=3, M=5, a_batch_stride=80, out_f32=True, ldc=32, c_batch_stride=999)


@case("gemm_pair", ws="fake")
@case("gemm_pair/no_ws")
def _(c, o):
    c.call("gemm_pair", dict(A=c.t("A0", 6, 16), W=c.t("W0", 24, 16)), dict(A=c.t("A1", 4, 8), W=c.t("W1", 12, 8), bias=c.t("b1", 12),
                                                                           out=c.t("o1", 4, 12)))
    c.call("gemm_pair", _gemm_full(c, "p", out_f32=False), _gemm_full(c, "q"))


def _qkv(c, tag="", fp8=False, full=False, **extra):
    dt = FP8 if fp8 else BF16
    H, Spad = 2, 16
    pos = [c.t("A" + tag, 8, 24, dtype=dt), c.t("W" + tag, 3 * H * 128, 24, dtype=dt)[:, :20] if full else c.t("W" + tag, 3 * H * 128, 24, dtype=dt),
           c.t("bias" + tag, 3 * H * 128) if full else None, c.t("Q" + tag, 1, H, Spad, 128), c.t("K" + tag, 1, H, Spad, 128),
           c.t("VT" + tag, 1, H, 128, Spad), c.t("nq" + tag, 128), c.t("nk" + tag, 128), c.t("cos" + tag, Spad, 128, dtype=F32),
           None if full else c.t("sin" + tag, Spad, 128, dtype=F32)]
    kw = dict(M=8, H=H, Spad=Spad, tok_off=0, rows_per_sample=8)
    if full:
        kw = dict(M=3, H=H, Spad=Spad, tok_off=5, rows_per_sample=3, batch=2, a_batch_stride=72, lda=22, a_offset=9, eps=1e-5, q_scale=0.125,
                  vt_perm=True)
    kw.update(extra)
    return pos, kw


@case("gemm_qkv", ws="fake")
@case("gemm_qkv/no_ws")
def _(c, o):
    pos, kw = _qkv(c)
    c.call("gemm_qkv", *pos, **kw)
    pos, kw = _qkv(c, "f", full=True, _act2=2, _bias2=c.t("b2", 768))
    c.call("gemm_qkv", *pos, **kw)


@case("gemm_qkv_pair", ws="fake")
@case("gemm_qkv_pair/no_ws")
def _(c, o):
    names = ("A", "W", "bias", "Q", "K", "VT", "norm_q", "norm_k", "cos", "sin")
    (p0, k0), (p1, k1) = _qkv(c, "0"), _qkv(c, "1", full=True, _act2=3, _bias2=c.t("b2", 768))
    c.call("gemm_qkv_pair", dict(zip(names, p0), **k0), dict(zip(names, p1), **k1))
    c.call("gemm_qkv_pair", dict(zip(names, p1), **k1), dict(zip(names, p0), **k0))


@case("gemm_fp8", ws="fake")
@case("gemm_fp8/no_ws")
def _(c, o):
    A8, W8 = c.t("A8", 6, 32, dtype=FP8), c.t("W8", 24, 32, dtype=FP8)
    c.call("gemm_fp8", A8, W8)
    c.call("gemm_fp8", A8, W8, c.t("bias", 24), batch=2, M=3, a_batch_stride=96, out_fp8=True)
    c.call("gemm_fp8", A8, W8, out_fp8=True, c_offset=5, out=c.t("o8", 200, dtype=FP8))
    c.call("gemm_fp8", c.t("A8f", 300, dtype=FP8), c.t("W8big", 8, 40, dtype=FP8)[:, :36], c.t("biasf", 8), c.t("outf", 300),
           M=5, N=6, K=33, batch=4, a_batch_stride=50, lda=34, a_offset=3, a_scale=c.t("as", 20, dtype=F32), a_scale_batch_stride=5,
           w_scale=c.t("wsc", 8, dtype=F32), alpha=0.75, c_batch_stride=60, ldc=18, c_offset=7, act=o.ACT_GELU_TANH, gate=c.t("gate", 4, 8),
           gate_batch_stride=8, res=c.t("res", 300), res_batch_stride=62, ldr=19, res_offset=11, out_fp8=False, out_inv_scale=0.5, _act2=1,
           _bias2=c.t("b2", 8))
    c.call("gemm_fp8", c.tensors["A8f"], c.tensors["W8big"], out=c.t("out8", 300, dtype=FP8), M=5, c_offset=7, res=c.tensors["res"], res_offset=11,
           out_fp8=True, out_inv_scale=2.0, alpha=3)


@case("gemm_qkv_fp8", ws="fake")
@case("gemm_qkv_fp8/no_ws")
def _(c, o):
    pos, kw = _qkv(c, fp8=True)
    c.call("gemm_qkv_fp8", *pos, **kw)
    pos, kw = _qkv(c, "f", fp8=True, full=True, a_scale=c.t("as", 6, dtype=F32), a_scale_batch_stride=3, w_scale=c.t("wsc", 768, dtype=F32), alpha=0.25)
    c.call("gemm_qkv_fp8", *pos, **kw)


@case("conv2d_nhwc")
@case("conv2d_nhwc/ws", ws="fake")     # the convolution never carries the stream-K workspace
def _(c, o):
    c.call("conv2d_nhwc", c.t("x", 2, 5, 6, 8), c.t("w", 16, 72), c.t("bias", 16), 5, 6, 8, 16, 3, 3, 1, 1)
    c.call("conv2d_nhwc", c.tensors["x"], c.t("w2", 16, 32), None, 5, 6, 8, 16, 2, 2, 2, 0)


def _conv_full(c, up, tag, **kw):
    d = dict(out=c.t("out" + tag, 4000), act=c.ops.ACT_RELU, bias2=c.t("bias2" + tag, 4, 16, dtype=F32)[:, :8], res=c.t("res" + tag, 4000), c_offset=5,
             c_batch_stride=900, ldc=24, res_offset=7, res_batch_stride=950, ldr=28, up=up, pad_w=2, B=4, a_batch_stride=130, a_offset=9, out_w=7,
             out_h=6, out_row_pitch=200, w_group=2)
    d.update(kw)
    return (c.t("x" + tag, 600), c.t("w" + tag, 2, 8, 3 * 2 * 4), c.t("bias" + tag, 2, 8), 5, 6, 4, 8, 3, 2, 1, 1), d


@case("conv2d_nhwc/full", ws="fake")
@case("conv2d_nhwc/full_no_ws")
def _(c, o):
    for i, up in enumerate((1, 2, True, False)):
        pos, kw = _conv_full(c, up, str(i))
        c.call("conv2d_nhwc", *pos, **kw)
    pos, kw = _conv_full(c, 1, "m", moments=c.t("mom", 4, 8, 2, dtype=F32))
    c.call("conv2d_nhwc", *pos, **kw)
    pos, kw = _conv_full(c, 2, "a", moments=c.t("moma", 4, 8, 2, dtype=F32), moments_accumulate=True)
    c.call("conv2d_nhwc", *pos, **kw)
    c.call("conv2d_nhwc", c.t("x", 2, 5, 6, 8), c.t("w", 16, 72), c.t("bias", 16), 5, 6, 8, 16, 3, 3, 1, 1, moments=c.tensors["mom"], up=True)
    c.call("conv2d_nhwc", c.tensors["x"], c.tensors["w"], None, 5, 6, 8, 16, 3, 3, 2, 1, res=c.t("r", 2, 3, 3, 16), pad_w=0, out_h=4)


@case("attention", ws="fake")
@case("attention/no_ws")
def _(c, o):
    Q, K, VT, out = c.t("Q", 1, 2, 16, 128), c.t("K", 1, 2, 16, 128), c.t("VT", 1, 2, 128, 16), c.t("out", 400)
    c.call("attention", Q, K, VT, out, 1, 2, 12, 16, 256, 3072, 0.088)
    c.call("attention", Q, K, VT, out, 1, 2, 12, 16, 260, 3100, 0.5, o_offset=13, vt_perm=True)
    c.call("attention", Q, K, VT, out, 1, 2, 12, 16, 260, 3100, 0.5, o_offset=13)
    c.call("attention_lse", Q, K, VT, out, c.t("lse", 1, 2, 16, dtype=F32), 1, 2, 12, 16, 256, 3072, 0.088)
    c.call("attention_lse", Q, K, VT, out, c.tensors["lse"], 1, 2, 12, 16, 260, 3100, 2, o_offset=17)
    out8 = c.t("out8", 400, dtype=FP8)
    c.call("attention_e4m3out", Q, K, VT, out8, 1, 2, 12, 16, 256, 3072, 0.088)
    c.call("attention_e4m3out", Q, K, VT, out8, 1, 2, 12, 16, 260, 3100, 0.5, o_offset=19, out_inv_scale=0.25)
    c.call("attention_prefers_vt_perm", 24, 4608, 0.088)
    Dv = c.t("Dv", 1, 2, 16, dtype=F32)
    c.call("attention_bwd", Q, K, c.t("V", 1, 2, 16, 128), c.t("QT", 1, 2, 128, 16), c.t("KT", 1, 2, 128, 16), c.t("dOh", 1, 2, 16, 128),
           c.t("dOT", 1, 2, 128, 16), c.tensors["lse"], Dv, c.t("dQ", 1, 2, 16, 128), c.t("dK", 1, 2, 16, 128), c.t("dV", 1, 2, 16, 128), 1, 2, 12, 16, 0.088)
    c.call("attention_bwd", Q, K, c.tensors["V"], None, None, c.tensors["dOh"], None, c.tensors["lse"], Dv, c.tensors["dQ"], c.tensors["dK"],
           c.tensors["dV"], 1, 2, 12, 16, 1, have_lse=True)
    c.call("attention_bwd_prep", c.t("dO", 400), out, Dv, 1, 2, 12, 16, do_bs=3072, lddo=256, o_bs=3100, ldo=260)
    c.call("attention_bwd_prep", c.tensors["dO"], out, Dv, 1, 2, 12, 16, do_bs=3072, lddo=256, o_bs=3100, ldo=260, do_offset=3, o_offset=5)


@case("qkv_split")
def _(c, o):
    n = [c.t("n%d" % i, 128) for i in range(4)]
    cos, sin = c.t("cos", 12, 128, dtype=F32), c.t("sin", 12, 128, dtype=F32)
    q0, q1 = c.t("qkv0", 4, 768), c.t("qkv1", 8, 768)
    Q, K, VT = c.t("Q", 1, 2, 16, 128), c.t("K", 1, 2, 16, 128), c.t("VT", 1, 2, 128, 16)
    c.call("qkv_split", q0, q1, 768, 770, 1, 12, 4, 2, *n, cos, sin, Q, K, VT, 16)
    c.call("qkv_split", q0, None, 768, 0, 1, 12, 4, 2, n[0], n[1], None, None, cos, sin, Q, K, VT, 16, eps=1e-5)
    d0, d1 = c.t("d0", 4, 768), c.t("d1", 8, 768)
    c.call("qkv_split_bwd", q0, q1, 768, 770, d0, d1, 772, 774, 1, 12, 4, 2, *n, cos, sin, Q, K, VT, 16)
    c.call("qkv_split_bwd", q0, q1, 768, 770, d0, d1, 772, 774, 1, 12, 4, 2, *n, cos, sin, Q, K, VT, 16, eps=1e-5)


@case("ln_modulate")
def _(c, o):
    X, Y, mod = c.t("X", 400), c.t("Y", 400), [c.t("m%d" % i, 2, 16, dtype=F32) for i in range(4)]
    c.call("ln_modulate", X, Y, 2, 6, 16, 2, *mod, 16)
    c.call("ln_modulate", X, Y, 2, 6, 16, 2, mod[0], mod[1], None, None, 16, eps=1e-5, x_bs=120, ldx=18, y_bs=130, ldy=20, x_offset=3, y_offset=5)
    Y8, rs = c.t("Y8", 400, dtype=FP8), c.t("rs", 12, dtype=F32)
    c.call("ln_modulate_fp8", X, Y, Y8, rs, 2, 6, 16, 2, *mod, 16)
    c.call("ln_modulate_fp8", X, None, Y8, rs, 2, 6, 16, 2, *mod, 16)
    c.call("ln_modulate_fp8", X, Y, Y8, rs, 2, 6, 16, 2, *mod, 16, eps=1e-5, x_bs=120, ldx=18, y_bs=130, ldy=20, x_offset=3, y_offset=5, y8_bs=140, ldy8=22,
           y8_offset=7)
    c.call("ln_affine", c.t("Xa", 3, 4, 16), c.t("w", 16), c.t("b", 16), 1e-5)
    c.call("ln_affine", c.tensors["Xa"], None, None, 1e-6, out=c.t("oa", 3, 4, 16))
    T, gate = c.t("T", 400), c.t("gate", 2, 16, dtype=F32)
    c.call("gated_residual_", X, T, gate, 2, 6, 16, 96, 16, 96, 16, 16)
    c.call("gated_residual_", X, T, gate, 2, 6, 16, 120, 18, 130, 20, 16, x_offset=3, t_offset=5)
    dY, dXin, dXout, part = c.t("dY", 400), c.t("dXin", 400), c.t("dXout", 400), c.t("part", 2, 2, 2, 16, dtype=F32)
    c.call("ln_mod_bwd", X, dY, mod[0], dXin, dXout, part, B=2, S=6, D=16, R=4)
    c.call("ln_mod_bwd", X, dY, mod[0], None, dXout, part, B=2, S=6, D=16, R=4, mult_is_scale=False, mult_bs=16, x_bs=120, ldx=18, dy_bs=130, ldy=20, dx_bs=140,
           lddx=22, x_offset=3, dy_offset=5, dx_offset=7, eps=1e-5)
    G, dT = c.t("G", 400), c.t("dT", 400)
    c.call("gate_bwd", X, T, gate, G, dT, part, B=2, S=6, D=16, R=4)
    c.call("gate_bwd", X, None, gate, None, dT, part, B=2, S=6, D=16, R=4, gate_bs=16, dx_bs=120, lddx=18, t_bs=130, ldt=20, g_bs=140, ldg=22, dt_bs=150,
           lddt=24, dx_offset=3, t_offset=5, g_offset=7, dt_offset=9)
    c.call("gate_bwd", X, T, gate, G, dT, part, B=2, S=6, D=16, R=4, t_offset=5, g_offset=7)


@case("skinny_linear")
def _(c, o):
    X, Xb, W, b = c.t("X", 2, 16, dtype=F32), c.t("Xb", 2, 16), c.t("W", 24, 16), c.t("b", 24)
    c.call("skinny_linear", X, W)
    c.call("skinny_linear", Xb, W, b, c.t("out", 2, 32, dtype=F32)[:, :24], o.ACT_SILU, o.ACT_GELU_TANH, True)
    c.call("skinny_linear", Xb, W, b, c.tensors["out"], ldy=48)
    Wg, bg = c.t("Wg", 3, 24, 16), c.t("bg", 3, 24)
    c.call("skinny_linear_grouped", X, Wg, rows=2)
    c.call("skinny_linear_grouped", c.t("X6", 6, 16), Wg, bg, rows=2, out=c.t("og", 6, 24, dtype=F32), act_in=o.ACT_SILU, act_out=o.ACT_RELU)
    c.call("skinny_linear_bwd", c.t("dy", 2, 24, dtype=F32), W)
    c.call("skinny_linear_bwd", c.tensors["dy"], W, chunk=10)
    c.call("linear_wgrad", c.tensors["dy"], X, c.t("dw", 24, 16, dtype=F32), c.t("db", 24, dtype=F32))
    c.call("linear_wgrad", c.tensors["dy"], X, c.tensors["dw"], None, act_in=o.ACT_SILU, accumulate=True)


@case("embeddings")
def _(c, o):
    c.call("timestep_sinusoid", c.t("t", 3, dtype=F32), 32)
    c.call("timestep_sinusoid", c.tensors["t"], 16, round_bf16=True)
    c.call("rope_table", c.t("ids", 5, 3, dtype=F32), (4, 6, 6))
    c.call("rope_table", c.tensors["ids"], (8,), theta=500.0)
    cos = torch.arange(40, dtype=F32).reshape(5, 8).div(2, rounding_mode="floor")
    pairs = c.call("rope_pairs", cos, cos + 1)
    assert torch.equal(pairs[..., 0], cos[:, 0::2]) and torch.equal(pairs[..., 1], cos[:, 0::2] + 1)
    with pytest.raises(ValueError):
        o.rope_pairs(torch.arange(40, dtype=F32).reshape(5, 8), cos)
    c.call("rope_pairs", torch.arange(40, dtype=F32).reshape(5, 8), cos, check=False)
    c.call("pad128", 129)
    x, eps = c.t("x", 2, 16), c.t("eps", 2, 16)
    c.call("euler_step_", x, eps, c.t("dt", 1, dtype=F32))
    c.call("to_bf16", c.t("f", 3, 5, dtype=F32))
    c.call("to_f32", c.t("h", 3, 5))
    c.call("seq_mean", c.t("sm", 2, 3, 8, dtype=F32))
    c.call("softmax_rows_", c.t("sr", 3, 4, 8))
    c.call("softmax_rows_", c.tensors["sr"], scale=0.5)
    c.call("transpose", c.t("tr", 2, 3, 8))
    c.call("transpose", c.t("tr1", 3, 8))
    c.call("transpose", c.t("trb", 400), c.t("tro", 400), batch=2, R=3, C=8, in_bs=30, ld_in=10, out_bs=40, ld_out=5, in_offset=3, out_offset=7)
    c.call("transpose", c.tensors["trb"], batch=2, R=3, C=8, in_bs=30)
    P, dP = c.t("P", 2, 8, 16), c.t("dP", 2, 8, 16)
    c.call("softmax_pad_", P, 2, 8, 6, 16, 12, 0.5)
    c.call("softmax_pad_", P, 2, 8, 6, 16, 12, 1, ld=20)
    c.call("softmax_bwd_", P, dP, 2, 8, 6, 16, 12, 0.5)
    c.call("softmax_bwd_", P, dP, 2, 8, 6, 16, 12, 1, ld=20)
    part, out = c.t("part", 400, dtype=F32), c.t("rout", 100, dtype=F32)
    c.call("reduce_rows", part, out, np_=4, len_=10)
    c.call("reduce_rows", part, out, np_=4, len_=10, nz=2, in_zs=50, in_ps=12, out_zs=11, accumulate=True, alpha=0.5, in_offset=3, out_offset=5)
    c.call("act_bwd_", c.t("dA", 3, 8), c.t("pre", 3, 8), o.ACT_SILU)
    c.call("act_bwd_", c.t("dAf", 3, 8, dtype=F32), c.t("pref", 3, 8, dtype=F32), o.ACT_GELU_ERF, rows=2, cols=6, ldd=8, ldp=9, d_offset=1, p_offset=2)
    c.call("kd_loss_rows", c.t("te", 3, 16), c.t("st", 3, 16), c.t("gr", 3, 16), c.t("rl", 3, dtype=F32), rows=3, D=12, temperature=2, loss_scale=0.5)
    c.call("kd_loss_rows", c.tensors["te"], c.tensors["st"], c.tensors["gr"], c.tensors["rl"], rows=3, D=12, temperature=2.5, loss_scale=1, ldt=16, lds=17, ldg=18)
    c.call("zero_if_nonfinite_", c.tensors["gr"], c.tensors["rl"])


@case("projector")
def _(c, o):
    x, w, b = c.t("x", 2, 3, 4, 8), c.t("w", 3, 25, dtype=F32), c.t("b", 1, dtype=F32)
    c.call("proj_conv5x5", x, w, b)
    c.call("proj_conv5x5", x, w, None, out=c.t("out", 2, 4, 8))
    table = c.call("proj_conv5x5_pack", w)
    c.tensors["table"] = table
    c.call("proj_conv5x5_packed", x, table, b)
    c.call("proj_conv5x5_packed", x, table, None, out=c.tensors["out"])
    with pytest.raises(ValueError):
        o.proj_conv5x5_packed(x, table[:2], b)
    c.call("proj_layer_mean", x, c.t("scale", 3, dtype=F32))
    c.call("proj_layer_mean", x, c.tensors["scale"], out=c.tensors["out"])
    dy = c.t("dy", 2, 4, 8)
    c.call("conv5x5_wgrad", x, dy)
    c.call("plane_dot", x, dy)
    c.call("plane_dot", x, dy, alpha=0.5, nchunk=8)


@case("reductions_and_optimizer")
def _(c, o):
    x, xb = c.t("x", 3, 7, dtype=F32), c.t("xb", 3, 7)
    c.call("sum_all", x)
    acc = c.call("sum_all", xb, squares=True, nblocks=16)
    c.tensors["acc"] = acc
    c.call("sum_all", x, out=acc, accumulate=True)
    coef = c.call("clip_coef", acc, 1.5)
    c.tensors["coef"] = coef
    p, g, m, v = c.t("p", 40), c.t("g", 40, dtype=F32), c.t("m", 40, dtype=F32), c.t("v", 40, dtype=F32)
    c.call("adamw_", p, g, m, v, lr=1e-3, beta1=0.9, beta2=0.99, eps=1e-8, weight_decay=0.01, step=3)
    c.call("adamw_", p, g, m, v, lr=1, beta1=0.5, beta2=0.75, eps=1e-6, weight_decay=0, step=1, coef=coef)
    table, cm, cv = c.t("table", 2, 2, dtype=I64), c.t("cm", 2, 256, dtype=U8), c.t("cv", 2, 256, dtype=U8)
    am, av, ms, mu = (c.t(n, k, dtype=F32) for n, k in (("am", 2), ("av", 2), ("ms", 256), ("mu", 256)))
    c.call("adamw8_", table, c.t("g8", 512, dtype=F32), cm, cv, am, av, ms, mu, lr=1e-3, beta1=0.9, beta2=0.99, eps=1e-8, weight_decay=0.01, step=3)
    c.call("adamw8_", table, c.tensors["g8"], cm, cv, am, av, ms, mu, lr=1, beta1=0.5, beta2=0.75, eps=1e-6, weight_decay=0, step=2, coef=coef)


@case("controlnext_forward")
def _(c, o):
    x, w, b = c.t("x", 2, 4, 6, 16), c.t("w", 4, 144), c.t("b", 4)
    c.call("conv3x3_narrow", x, w, b, 3)
    c.call("conv3x3_narrow", x, w, None, 4, out=c.t("on", 2, 4, 6, 8), ldy=8)
    img, wi = c.t("img", 2, 3, 4, 6), c.t("wi", 16, 3, 3, 3)
    c.call("conv3x3_image", img, wi, c.t("bi", 16))
    c.call("conv3x3_image", img, wi, None, moments=c.t("mom", 2, 16, 2, dtype=F32))
    params = c.t("params", 2, 4, 6, 8)
    c.call("vae_posterior", params, 4)
    c.call("vae_posterior", params, 4, eps=c.t("veps", 2, 4, 4, 6), scale_shift=(0.1159, 0.3611), packed=True)
    c.call("vae_posterior", c.t("params2", 2, 4, 6, 12)[..., :8], 4, scale_shift=(0.5, 2))
    c.call("conv_stem", c.t("xs", 2, 8, 6, 3), c.t("ws", 16, 3, 3, 3, dtype=F32), c.t("bs", 16, dtype=F32), 16)
    gw, gb = c.t("gw", 2, 16), c.t("gb", 2, 16)
    c.call("groupnorm_nhwc", x, gw[1], gb[1], 4, 1e-5)
    c.call("groupnorm_nhwc", x, gw, gb, 2, 1e-6, act=o.ACT_SILU, pre_add=c.t("pre", 2, 16, dtype=F32), post_add=c.t("post", 2, 4, 6, 16),
           out=c.t("og", 2, 4, 6, 16), w_group=1)
    mom = c.call("groupnorm_moments", x)
    c.tensors["gmom"] = mom
    c.call("groupnorm_nhwc_from_moments", x, mom, gw[0], gb[0], 4, 1e-5)
    c.call("groupnorm_nhwc_from_moments", x, mom, gw, gb, 2, 1e-6, act=o.ACT_SILU, pre_add=c.tensors["pre"], post_add=c.tensors["post"], out=c.tensors["og"],
           w_group=1)
    c.call("quantize_rows_fp8", c.t("q", 3, 5, 16))
    c.call("quantize_rows_fp8", c.t("qv", 6, 24)[:, :16], static_inv_scale=0.5)
    c.call("quantize_rows_fp8", c.t("q1", 16))


@case("controlnext_backward")
def _(c, o):
    """the caller-owned f32 scratch of the backward entry points: the stub answers 96, 40, 160 floats -- one growing buffer per kind"""
    x, dy = c.t("x", 2, 5, 6, 8), c.t("dy", 2000)
    dw, db = c.t("dw", 16, 8, 3, 3, dtype=F32), c.t("db", 16, dtype=F32)
    c.call("conv_wgrad_workspace_floats", 2, 5, 6, 8, 16, 3, 3)
    c.call("conv_wgrad", x, dy, dw, db, 5, 6, 8, 5, 6, 16, 3, 3, 1, 1)
    c.call("conv_wgrad", x, dy, dw, None, 5, 6, 8, 5, 6, 16, 3, 3, 1, 1, B=1, dy_offset=3, dy_batch_stride=700, ldy=20, accumulate=True)
    c.call("conv_wgrad", x, dy, dw, db, 5, 6, 8, 5, 6, 16, 3, 3, 1, 1)
    xs, dys, dws = c.t("xs", 2, 8, 6, 3), c.t("dys", 2, 4, 3, 16), c.t("dws", 16, 3, 3, 3, dtype=F32)
    for kw in ({}, {"accumulate": True}, {}, {}):
        c.call("conv_stem_wgrad", xs, dys, dws, None if kw else db, **kw)
    g = c.t("g", 2, 5, 6, 8)
    c.call("groupnorm_bwd", x, g, c.t("gw", 8), c.t("gb", 8), 2, 1e-5)
    c.call("groupnorm_bwd", x, g, c.tensors["gw"], c.tensors["gb"], 4, 1e-6, act=o.ACT_SILU, pre_add=c.t("pre", 2, 8, dtype=F32),
           dpre=c.t("dpre", 2, 8, dtype=F32), dx_in=c.t("dxin", 2, 5, 6, 8), dx=c.t("dx", 2, 5, 6, 8), dw=c.t("dgw", 8, dtype=F32),
           db=c.t("dgb", 8, dtype=F32), in_relu=True, accumulate=True)
    c.call("groupnorm_bwd", x, g, c.tensors["gw"], c.tensors["gb"], 2, 1e-5)
    lat, noise, sigma = c.t("lat", 2, 4, 4, 6), c.t("noise", 2, 4, 4, 6), c.t("sigma", 2, dtype=F32)
    c.call("flow_match_noise", lat, noise, sigma)
    c.call("flow_match_noise", lat, noise, sigma, noisy=c.t("noisy", 2, 6, 16), target=c.t("target", 2, 6, 16))
    pred, tgt = c.t("pred", 2, 6, 16), c.tensors["target"]
    c.call("mse_loss_workspace_floats", 192)
    c.call("mse_loss_grad", pred, tgt)
    c.call("mse_loss_grad", pred, tgt, grad_scale=0.5, d_pred=c.t("dpred", 2, 6, 16), loss=c.t("loss", 1, dtype=F32))
    c.call("mse_loss_grad", pred, tgt)


@case("scratch_sizes")
def _(c, o):
    """group-norm scratch by exact size, the conv moments' one growing buffer, fresh moments scratch per call: three rounds of the stub's sizes"""
    x, w, b = c.t("x", 2, 4, 6, 16), c.t("w", 16), c.t("b", 16)
    mom = c.t("mom", 2, 16, 2, dtype=F32)
    cw, img, wi = c.t("cw", 16, 144), c.t("img", 2, 3, 4, 6), c.t("wi", 16, 3, 3, 3)
    for _ in range(3):
        c.call("groupnorm_nhwc", x, w, b, 4, 1e-5)
        c.call("groupnorm_nhwc_from_moments", x, mom, w, b, 4, 1e-5)
        c.call("groupnorm_moments", x)
        c.call("conv2d_nhwc", x, cw, None, 4, 6, 16, 16, 3, 3, 1, 1, moments=mom)
        c.call("conv3x3_image", img, wi, None, moments=mom)


@case("library_state")
def _(c, o):
    def option():
        with o.option("gemm_tile", 256):
            return o.option_epoch()

    def streamk_scope():
        with o.streamk_scope("a workspace") as ws:
            return ws

    c.call("option_epoch")
    c.call(option)
    c.call("option_epoch")
    c.call(streamk_scope)
    c.call("streamk_poll")
    c.call("streamk_check")
    c.call("streamk_check", sync=False)
    ws = c.call(o.StreamKWorkspace, device=torch.device("cpu"))
    assert ws.nbytes == WS_BYTES == ws.buf.numel() and ws.buf.dtype == U8 and ws.marker.data_ptr() == ws.buf.data_ptr() + 4 * o.SK_ERR_SLOT
    c.tensors["skws"] = ws.buf
    c.call(ws.check)
    c.call(ws.check, sync=True)
    c.call("streamk_check")
    c.call("streamk_check", sync=False)


# wrappers that a case of another name calls
COVERED_BY = {"attention": ["attention_lse", "attention_e4m3out", "attention_prefers_vt_perm", "attention_bwd", "attention_bwd_prep"],
              "qkv_split": ["qkv_split_bwd"],
              "ln_modulate": ["ln_modulate_fp8", "ln_affine", "gated_residual_", "ln_mod_bwd", "gate_bwd"],
              "skinny_linear": ["skinny_linear_grouped", "skinny_linear_bwd", "linear_wgrad"]}


def run_case(name, monkeypatch):
    from x2i_amd import _lib
    fn, ws = CASES[name]
    rec = Recorder(_lib.SIGNATURES)
    monkeypatch.setattr(_lib, "load", lambda: rec)
    monkeypatch.setattr(_lib, "_option_epoch", 0)
    ops = fresh_ops()
    c = Case(ops, rec)
    fake = FakeWorkspace(c) if ws == "fake" else None
    monkeypatch.setattr(ops, "_req", lambda t, dtype, name: None)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "_sk_workspace", lambda: fake)
    fn(c, ops)
    return c.out


def surface():
    """public names of ops (modules aside) and the signature of every public callable"""
    ops = fresh_ops()
    names = sorted(n for n, v in vars(ops).items() if not n.startswith("_") and not isinstance(v, types.ModuleType))
    sigs = {}
    for n in names:
        v = getattr(ops, n)
        if callable(v):
            try:
                sigs[n] = str(inspect.signature(v))
            except ValueError:   # ctypes structures
                sigs[n] = "(...)"
            if inspect.isclass(v):
                sigs[n] = {m: str(inspect.signature(f)) for m, f in sorted(vars(v).items()) if inspect.isfunction(f)} or sigs[n]
    return {"names": names, "signatures": sigs}


def wrappers():
    ops = fresh_ops()
    return sorted(n for n, v in vars(ops).items() if not n.startswith("_") and inspect.isfunction(v) and v.__module__ == ops.__name__)


def record(monkeypatch):
    return {"surface": surface(), "cases": {name: run_case(name, monkeypatch) for name in CASES}}


def expected():
    with open(TRACE) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_wrapper_hands_the_library_what_it_did(name, monkeypatch):
    got = json.loads(json.dumps(run_case(name, monkeypatch)))
    want = expected()["cases"][name]
    assert [g["fn"] for g in got] == [w["fn"] for w in want]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s, call %d (%s)" % (name, i, g["fn"])


def test_public_surface_of_ops_is_unchanged():
    got, want = json.loads(json.dumps(surface())), expected()["surface"]
    assert got["names"] == want["names"]
    for n in want["signatures"]:
        assert got["signatures"][n] == want["signatures"][n], n


def test_every_public_wrapper_is_traced(monkeypatch):
    want = expected()
    assert sorted(want["cases"]) == sorted(CASES)
    called = {e["fn"] for entries in want["cases"].values() for e in entries}
    for group, names in COVERED_BY.items():
        assert group in CASES and set(names) <= called
    assert not set(wrappers()) - called, set(wrappers()) - called
    twice = ("gemm", "gemm_pair", "gemm_qkv", "gemm_qkv_pair", "gemm_fp8", "gemm_qkv_fp8", "conv2d_nhwc")
    for n in twice:
        assert sum(e["fn"] == n for entries in want["cases"].values() for e in entries) >= 2, n
    # both workspace cases: set from the fake workspace, zero without; the convolution never carries one
    def workspaces(case_name, export):
        return [a["workspace"] for e in want["cases"][case_name] for ex, args in e["calls"] if ex == export for a in args[:1]]
    assert set(map(str, workspaces("gemm/ws", "x2i_gemm_bf16"))) == {str(["ws", 0])} and set(workspaces("gemm", "x2i_gemm_bf16")) == {None}
    assert set(workspaces("conv2d_nhwc/ws", "x2i_conv2d_nhwc_bf16")) == {None} == set(workspaces("conv2d_nhwc/full", "x2i_conv2d_nhwc_bf16"))
    assert os.path.getsize(TRACE) < 200 * 1024


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_ops_abi_cpu.py --record")
    mp = pytest.MonkeyPatch()
    try:
        trace = record(mp)
    finally:
        mp.undo()
    def dumps(v):
        return json.dumps(v, sort_keys=True, separators=(",", ":"))

    with open(TRACE, "w") as f:   # one line per case
        f.write('{"cases":{\n' + ",\n".join("%s:%s" % (dumps(n), dumps(t)) for n, t in sorted(trace["cases"].items())))
        f.write('\n},\n"surface":%s}\n' % dumps(trace["surface"]))
    print("%s: %d cases, %d bytes" % (TRACE, len(trace["cases"]), os.path.getsize(TRACE)))
