"""Record the bf16 GEMM launches a module makes and replay each one on fresh operands against the float64 reference of tests/gemm_ref.py:
the recorder and the replayer shared by tests/test_gemm_fp64_gpu.py (a FLUX denoise step) and tests/test_encoder_gemm_fp64_gpu.py (the
encoder and decoder modules).  No GPU-only imports at module level.

record(ops, run) replaces ops.gemm / gemm_pair / gemm_qkv / gemm_qkv_pair by a recorder while run() runs the module (the modules call them
through the ops module) and keeps, per call, the geometry of every tensor argument (its storage's identity and size, dtype, shape, strides,
offset) and every scalar.  replay(ops, rec, name, kind, seed) makes the same ops call with the recorded geometry -- every shape, stride and
offset, the storages shared as the module shares them -- on fresh storages filled with one operand kind (gemm_ref.KINDS), outputs starting as
the sentinel, and checks every output element and that nothing outside the output views was written.

What a replay understands beyond the FLUX step's launches:
  a weight per item    w_batch_stride != 0: W of item z is W.as_strided((N, K), (ldw, 1), offset + z * w_batch_stride); the reference gets
                       [batch, N, K].  a_batch_stride = 0 with batch > 1 is one A shared by the items (and tagged once).
  overlapping A rows   lda < K (a stride-2 convolution as a GEMM): the storage is filled, not the view, and `tagged` scales the storage
                       (gemm_ref.tag_scales_flat); the reference reads A through the strided view the kernel gets.
  res aliasing out     out=X, res=X: the residual is filled into the shared storage, a clone of it is what the reference reads, and the
                       untouched-memory mask comes from the output view alone.
  an output the call allocates (out=None) is recorded from what the call returned and replayed as an explicit `out`."""
import math

import torch

from tests import gemm_ref as R

DEV = "cuda"
TENSOR_ARGS = ("A", "W", "bias", "out", "res", "gate", "out2", "bias2", "Q", "K", "VT", "norm_q", "norm_k", "cos", "sin")
OUTPUT_ROLES = ("out", "res", "out2", "Q", "K", "VT")
ACT_NAMES = {R.ACT_NONE: "", R.ACT_GELU_TANH: "gelu_tanh", R.ACT_GELU_ERF: "gelu_erf", R.ACT_SILU: "silu", R.ACT_RELU: "relu"}


# ---------------------------------------------------------------------------------------------------------------- recording
class Spec:
    """geometry of one tensor argument: its storage (identity and size), dtype, shape, strides, offset"""

    def __init__(self, t, keep=False):
        self.key = t.untyped_storage().data_ptr()
        self.numel = t.untyped_storage().nbytes() // t.element_size()
        self.dtype, self.shape, self.stride, self.offset = t.dtype, tuple(t.shape), tuple(t.stride()), t.storage_offset()
        self.obj = t if keep else None          # (kept for the RoPE tables only: the replay reads the model's own)


def _record(kw):
    return {k: (Spec(v, keep=k in ("cos", "sin")) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}


def record(ops, run):
    """[(op name, [problem dict])] of the ops.gemm* calls that run() makes, in order, with the module's scalars.  Every tensor the calls saw
    stays alive until run() is over: no storage is freed and reused while the recording names storages by address."""
    calls, alive = [], []
    names = {"gemm": lambda *a, **k: [_record(dict(zip(("A", "W", "bias", "out"), a), **k))],
             "gemm_pair": lambda g0, g1: [_record(g0), _record(g1)],
             "gemm_qkv": lambda *a, **k: [_record(dict(zip(("A", "W", "bias", "Q", "K", "VT", "norm_q", "norm_k", "cos", "sin"), a), **k))],
             "gemm_qkv_pair": lambda g0, g1: [_record(g0), _record(g1)]}
    orig = {n: getattr(ops, n) for n in names}

    def wrap(n):
        def f(*a, **k):
            probs = names[n](*a, **k)
            calls.append((n, probs))
            alive.extend(list(a) + list(k.values()))
            ret = orig[n](*a, **k)
            if n == "gemm" and probs[0].get("out") is None:      # the call allocated its output: dense [batch, M, N]
                alive.append(ret)
                probs[0]["out"] = Spec(ret)
                if probs[0].get("batch", 1) > 1:
                    probs[0]["c_batch_stride"] = ret.stride(0)
            return ret
        return f
    try:
        for n in names:
            setattr(ops, n, wrap(n))
        run()
        torch.cuda.synchronize()
    finally:
        for n, f in orig.items():
            setattr(ops, n, f)
    del alive
    return calls


def geometry(p, qkv=False):
    """(batch, M, N, K, lda, ldc) of a recorded problem, with the defaults ops.gemm applies"""
    A, W = p["A"], p["W"]
    batch = p.get("batch", 1)
    M = p.get("M") or math.prod(A.shape[:-1])
    K = W.shape[-1] if qkv or p.get("K") is None else p["K"]      # (a QKV problem's "K" is the K output)
    N = (3 * p["H"] * 128) if qkv else (p.get("N") or W.shape[-2])
    return batch, M, N, K, p.get("lda") or A.shape[-1], p.get("ldc") or N


def describe(p):
    """a recorded ops.gemm problem in words: 'MxNxK' (batch first where there is one) and what the launch uses beyond plain A W^T + b"""
    batch, M, N, K, lda, ldc = geometry(p)
    s = ("%dx" % batch if batch > 1 else "") + "%dx%dx%d" % (M, N, K)
    out, res = p["out"], p.get("res")
    flags = [ACT_NAMES[p.get("act", 0)],
             "bias" if p.get("bias") is not None else "",
             "gate" if p.get("gate") is not None else "",
             ("res_inplace" if res.key == out.key else "res") if res is not None else "",
             "ldr" if res is not None and p.get("ldr") is not None else "",
             "a_off" if p.get("a_offset") else "",
             "lda%d" % lda if lda != K else "",
             "c_off" if p.get("c_offset") else "",
             "ldc%d" % ldc if ldc != N else "",
             "wbatch" if p.get("w_batch_stride") else "",
             "shared_a" if batch > 1 and not p.get("a_batch_stride") else "",
             "f32" if p.get("out_f32") else "",
             "out2_" + ACT_NAMES[p.get("act2", 0)] if p.get("out2") is not None else ""]
    return " ".join([s] + [f for f in flags if f])


def named(calls):
    """{'calls': calls, 'names': one name per call: its index and, for a plain gemm, describe() of it}"""
    names = ["%02d %s" % (i, describe(probs[0]) if op == "gemm" else op) for i, (op, probs) in enumerate(calls)]
    return dict(calls=calls, names=names)


# ---------------------------------------------------------------------------------------------------------------- replay
def _fill(role, spec, gen):
    n = spec.numel
    if role in OUTPUT_ROLES:
        return R.poison_(torch.empty(n, device=DEV, dtype=spec.dtype))
    if role in ("norm_q", "norm_k"):
        return (1.0 + 0.1 * torch.randn(n, device=DEV, generator=gen)).to(spec.dtype)
    scale = {"A": 1.0, "W": 0.02, "bias": 0.5, "gate": 1.0, "bias2": 0.5}[role]
    return (scale * torch.randn(n, device=DEV, generator=gen)).to(spec.dtype)


def _view(buf, spec):
    return buf.as_strided(spec.shape, spec.stride, spec.offset)


def _tag_A(buf, A3, off, batch, M, Kd, lda, a_bs):
    """the `tagged` kind on A, once per distinct item (a shared A -- a_batch_stride = 0 -- is one item)"""
    items = batch if a_bs else 1
    if lda >= Kd:
        for z in range(items):
            A3[z].copy_((A3[z].double() * R.tag_scales(M, Kd, z, device=DEV)).to(A3.dtype))
        return
    n = (M - 1) * lda + Kd                        # overlapping rows: copy_ into the view is refused; scale the items' flat storage
    assert items == 1 or a_bs >= n, "items that overlap in memory"
    for z in range(items):
        flat = buf[off + z * a_bs:off + z * a_bs + n]
        flat.copy_((flat.double() * R.tag_scales_flat(n, lda, z, device=DEV)).to(flat.dtype))


def replay(ops, rec, name, kind, seed):
    """Replay the launch `name` of the recording on fresh `kind` operands; check every element and the sentinels.  Returns (form, worst share)."""
    from x2i_amd import _lib
    op, probs = rec["calls"][rec["names"].index(name)]
    gen = torch.Generator(device=DEV).manual_seed(seed)
    bufs, first_role = {}, {}
    for p in probs:
        for role in TENSOR_ARGS:
            s = p.get(role)
            if isinstance(s, Spec) and role not in ("cos", "sin"):
                if s.key not in bufs:
                    bufs[s.key] = _fill(role, s, gen)
                    first_role[s.key] = role
                # a storage is all operands or all outputs: an operand inside an output's storage would break the sentinel outside the views
                assert (role in OUTPUT_ROLES) == (first_role[s.key] in OUTPUT_ROLES), (name, role, first_role[s.key])
    qkv = op.startswith("gemm_qkv")
    launch_args, checks, masks = [], [], {}
    for p in probs:
        kw = {k: v for k, v in p.items() if not isinstance(v, Spec)}
        t = {r: (_view(bufs[s.key], s) if r not in ("cos", "sin") else s.obj) for r, s in p.items() if isinstance(s, Spec)}
        Aspec, Wspec = p["A"], p["W"]
        batch, M, N, Kd, lda, ldc = geometry(p, qkv)
        a_bs, w_bs = p.get("a_batch_stride", 0), p.get("w_batch_stride", 0)
        a_off = Aspec.offset + p.get("a_offset", 0)
        A3 = bufs[Aspec.key].as_strided((batch, M, Kd), (a_bs, lda, 1), a_off)
        if w_bs:                                  # a weight per item
            Wv = bufs[Wspec.key].as_strided((batch, N, Kd), (w_bs, Wspec.stride[-2], 1), Wspec.offset)
        else:
            Wv = bufs[Wspec.key].as_strided((N, Kd), (Wspec.stride[-2], 1), Wspec.offset)
        W_of = (lambda z, Wv=Wv: Wv[z]) if w_bs else (lambda z, Wv=Wv: Wv)
        bias = t["bias"].reshape(-1)[:N] if "bias" in t else None
        assert p.get("bias2") is None and not p.get("w_group"), "not replayed: bias2 / grouped weights"
        if kind == "tagged":
            _tag_A(bufs[Aspec.key], A3, a_off, batch, M, Kd, lda, a_bs)
        chk = dict(qkv=qkv, A3=A3, W=Wv, bias=bias, M=M, N=N, batch=batch, p=p, t=t)
        if not qkv:
            out = p["out"]
            c_bs = p.get("c_batch_stride", 0)
            c_view = ((batch, M, N), (c_bs, ldc, 1), out.offset + p.get("c_offset", 0))
            chk["C3"] = bufs[out.key].as_strided(*c_view)
            masks.setdefault(out.key, []).append(c_view)            # (the mask: the output views alone, also where res shares the storage)
            if "out2" in t:
                c2_view = ((batch, M, N), (c_bs, ldc, 1), p["out2"].offset + p.get("c_offset", 0))
                chk["C2"] = bufs[p["out2"].key].as_strided(*c2_view)
                masks.setdefault(p["out2"].key, []).append(c2_view)
            if "gate" in t:
                gs = p["gate"]
                chk["gate"] = bufs[gs.key].as_strided((batch, N), (p.get("gate_batch_stride", 0), 1), gs.offset)
            if "res" in t:
                rs = p["res"]
                r_view = ((batch, M, N), (p.get("res_batch_stride", 0), p.get("ldr") or ldc, 1), rs.offset + p.get("res_offset", 0))
                if rs.key == out.key:             # in place: the kernel reads an element's residual and writes the element, nothing else
                    assert r_view == c_view, (name, r_view, c_view)
                res3 = bufs[rs.key].as_strided(*r_view)
                for z in range(batch):
                    for r0 in range(0, M, R.ROWS):
                        r1 = min(M, r0 + R.ROWS)
                        if kind == "cancel":       # res = -gate * act(lin): the output is the tiny rounding residual of res
                            lin, _ = R.linear_f64(A3[z, r0:r1], W_of(z), bias)
                            gz = chk["gate"][z].double() if "gate" in chk else 1.0
                            res3[z, r0:r1] = (-gz * R.act_f64(lin, p.get("act", 0))).to(res3.dtype)
                            del lin
                        else:
                            res3[z, r0:r1] = (R.lin_scale(Kd) * torch.randn((r1 - r0, N), device=DEV, generator=gen)).to(res3.dtype)
                chk["res"] = res3.clone()         # what the reference reads: the residual as it was before the launch
        checks.append(chk)
        # the tensors of the call itself: the recorded views on the fresh storages
        args = dict(kw)
        args.update({r: v for r, v in t.items()})
        launch_args.append(args)
    fn = getattr(ops, op)
    if op in ("gemm_pair", "gemm_qkv_pair"):
        fn(launch_args[0], launch_args[1])
    else:
        fn(**launch_args[0])
    form = int(_lib.get_option("last_gemm_tile"))
    torch.cuda.synchronize()
    worst = 0.0
    for i, c in enumerate(checks):
        p, t = c["p"], c["t"]
        rep = R.Report(f"{name}[{i}] {kind}")
        if c["qkv"]:
            R.check_qkv(rep, c["A3"], c["W"], c["bias"], t["norm_q"].reshape(-1)[:128], t["norm_k"].reshape(-1)[:128], t["cos"], t.get("sin"),
                        t["Q"], t["K"], t["VT"], H=p["H"], tok_off=p["tok_off"], rows_per_sample=p["rows_per_sample"],
                        q_scale=p.get("q_scale", 1.0), eps=p.get("eps", 1e-6), vt_perm=bool(p.get("vt_perm", False)))
        else:
            R.check_gemm(rep, c["A3"], c["W"], c["bias"], c["C3"], act=p.get("act", 0), gate=c.get("gate"), res=c.get("res"),
                         C2=c.get("C2"), act2=p.get("act2", 0), out_f32=bool(p.get("out_f32", False)))
        worst = max(worst, rep.done())
    if qkv:
        p, t = checks[0]["p"], checks[0]["t"]
        R.check_qkv_padding(f"{name} {kind}", t["Q"], t["K"], t["VT"], rec["S"], bool(p.get("vt_perm", False)))
    for key, views in masks.items():
        buf = bufs[key]
        R.check_untouched(f"{name} {kind}", buf, R.write_mask(buf, views), row_len=views[0][1][1])
    del bufs, checks
    return form, worst
