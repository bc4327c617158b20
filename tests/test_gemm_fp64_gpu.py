"""Every bf16 GEMM launch of a denoise step, at the model's shapes, against the float64 reference of tests/gemm_ref.py -- every output element
of every launch, and the sentinel outside what the launch may write.

The launch list is taken from the model, not copied by hand: a full-width FluxTransformer2DModel (D = 3072, H = 24) with one double and one
single block runs prepare_conditioning and one denoise with ops.gemm / gemm_pair / gemm_qkv / gemm_qkv_pair replaced by a recorder
(x2i_amd/flux.py calls them through the ops module).  Each recorded launch is then replayed through the same ops call with the recorded
geometry (every shape, stride and offset, the storages shared as the model shares them) on fresh buffers filled with each operand kind
(gemm_ref.KINDS); outputs start as the sentinel, the RoPE tables are the model's.  The launches of one configuration run kind after kind, so a
launch that takes stream-K or FX always follows one of its own geometry on other inputs: a stale slab or flag would show.

Configurations (B, image side): (1, 512) -- FX takes proj_out and the ff.2 pair by default; (1, 1024) -- 216 whole tiles; (4, 1024) -- the
bench configuration, stream-K chains; (2, 1008) -- Si = 3969: ragged M and tile counts not multiples of 8.  St = 512 throughout.  The
alternative kernel forms (gemm_fx 0 / 1, gemm_streamk 0, gemm_persist 0, gemm_w4 0, gemm_pair 0, gemm_tile 128) replay one configuration
each, and every launch's form is read back through last_gemm_tile (3256 FX, 2256 grouped, 1256 peeled tail, 256, 128, 0 generic)."""
import time

import pytest
import torch

from tests import gemm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ST = 512
CONFIGS = {"b1_512": (1, 512), "b1_1024": (1, 1024), "b4_1024": (4, 1024), "b2_1008": (2, 1008)}
LAUNCHES = ["context_embedder", "x_embedder", "qkv_pair", "to_out_pair", "ff0_pair", "ff2_pair", "single_qkv", "proj_mlp", "single_proj_out",
            "final_proj_out"]
OPS = ["gemm", "gemm", "gemm_qkv_pair", "gemm_pair", "gemm_pair", "gemm_pair", "gemm_qkv", "gemm", "gemm", "gemm"]


def forms(*tiles):
    return dict(zip(LAUNCHES, tiles))


# the kernel form of every launch (last_gemm_tile after the call; for a pair not grouped: its second launch's), measured on MI355X:
#                             context x_emb  qkv   to_out ff.0  ff.2  s.qkv  mlp   s.proj f.proj
DEFAULT_FORMS = {"b1_512": forms(128, 128, 2256, 2256, 2256, 3256, 256, 1256, 3256, 128),
                 "b1_1024": forms(128, 256, 2256, 2256, 2256, 2256, 256, 256, 256, 128),
                 "b4_1024": forms(128, 256, 2256, 2256, 2256, 2256, 256, 256, 256, 128),
                 "b2_1008": forms(128, 256, 2256, 2256, 2256, 2256, 1256, 256, 256, 128)}
ALT_FORMS = [("b1_512", "gemm_fx", 0, forms(128, 128, 2256, 2256, 2256, 2256, 256, 1256, 128, 128)),
             ("b1_512", "gemm_fx", 1, DEFAULT_FORMS["b1_512"]),
             ("b1_512", "gemm_persist", 0, forms(128, 128, 128, 128, 128, 128, 256, 1256, 128, 128)),
             ("b1_512", "gemm_w4", 0, forms(128, 128, 128, 128, 128, 128, 256, 1256, 128, 128)),
             ("b1_512", "gemm_pair", 0, forms(128, 128, 128, 128, 128, 128, 256, 1256, 3256, 128)),
             ("b1_512", "gemm_tile", 128, forms(*[128] * 10)),
             ("b4_1024", "gemm_streamk", 0, forms(128, 256, 2256, 2256, 2256, 2256, 1256, 1256, 1256, 128))]
TENSOR_ARGS = ("A", "W", "bias", "out", "res", "gate", "out2", "bias2", "Q", "K", "VT", "norm_q", "norm_k", "cos", "sin")
WORST = {}      # launch -> worst share of the f32 allowance used, over everything this module ran (printed by each test)


@pytest.fixture(scope="module")
def ops():
    from x2i_amd import ops as o
    o._lib.load()
    return o


@pytest.fixture
def opt(ops):
    from x2i_amd import _lib
    saved = {}

    def set_(name, value):
        old = _lib.set_option(name, value)
        saved.setdefault(name, old)
    yield set_
    for k, v in saved.items():
        _lib.set_option(k, v)


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


_recordings = {}


def recording(ops, cfg):
    """[(op name, [problem dict])] of one prepare_conditioning + denoise at configuration cfg, with the model's scalars"""
    if cfg in _recordings:
        return _recordings[cfg]
    from x2i_amd.flux import FluxTransformer2DModel
    B, side = CONFIGS[cfg]
    hw = side // 16
    Si = hw * hw
    m = FluxTransformer2DModel(num_layers=1, num_single_layers=1, device=DEV).init_random_(seed=3)
    g = torch.Generator().manual_seed(5)
    enc = torch.randn((B, ST, 4096), generator=g).to(DEV, torch.bfloat16)
    pooled = torch.randn((B, 768), generator=g).to(DEV, torch.bfloat16)
    txt_ids = torch.zeros((ST, 3))
    img_ids = torch.zeros((hw, hw, 3))
    img_ids[..., 1] += torch.arange(hw)[:, None]
    img_ids[..., 2] += torch.arange(hw)[None, :]
    hs = torch.randn((B, Si, 64), generator=g).to(DEV, torch.bfloat16)
    calls, alive = [], []
    names = {"gemm": lambda *a, **k: [_record(dict(zip(("A", "W", "bias", "out"), a), **k))],
             "gemm_pair": lambda g0, g1: [_record(g0), _record(g1)],
             "gemm_qkv": lambda *a, **k: [_record(dict(zip(("A", "W", "bias", "Q", "K", "VT", "norm_q", "norm_k", "cos", "sin"), a), **k))],
             "gemm_qkv_pair": lambda g0, g1: [_record(g0), _record(g1)]}
    orig = {n: getattr(ops, n) for n in names}

    def wrap(n):
        def f(*a, **k):
            calls.append((n, names[n](*a, **k)))
            alive.extend(list(a) + list(k.values()))     # (no storage is freed and reused while the recording names storages by address)
            return orig[n](*a, **k)
        return f
    try:
        for n in names:
            setattr(ops, n, wrap(n))
        state = m.prepare_conditioning(enc, pooled, txt_ids.to(DEV), img_ids.reshape(-1, 3).to(DEV))
        m.denoise(state, hs, torch.full((B,), 0.75, device=DEV))
        torch.cuda.synchronize()
    finally:
        for n, f in orig.items():
            setattr(ops, n, f)
    S = ST + Si
    rec = dict(calls=calls, B=B, Si=Si, S=S)
    del m, state, alive
    _recordings.clear()
    _recordings[cfg] = rec
    return rec


# ---------------------------------------------------------------------------------------------------------------- replay
def _fill(role, spec, gen):
    n = spec.numel
    if role in ("out", "res", "out2", "Q", "K", "VT"):
        return R.poison_(torch.empty(n, device=DEV, dtype=spec.dtype))
    if role in ("norm_q", "norm_k"):
        return (1.0 + 0.1 * torch.randn(n, device=DEV, generator=gen)).to(spec.dtype)
    scale = {"A": 1.0, "W": 0.02, "bias": 0.5, "gate": 1.0, "bias2": 0.5}[role]
    return (scale * torch.randn(n, device=DEV, generator=gen)).to(spec.dtype)


def _view(buf, spec):
    return buf.as_strided(spec.shape, spec.stride, spec.offset)


def replay(ops, rec, idx, kind, seed):
    """Replay launch idx of the recording on fresh `kind` operands; check every element and the sentinels.  Returns (form, worst share)."""
    from x2i_amd import _lib
    op, probs = rec["calls"][idx]
    name = LAUNCHES[idx]
    gen = torch.Generator(device=DEV).manual_seed(seed)
    bufs = {}
    for p in probs:
        for role in TENSOR_ARGS:
            s = p.get(role)
            if isinstance(s, Spec) and s.key not in bufs and role not in ("cos", "sin"):
                bufs[s.key] = _fill(role, s, gen)
    qkv = op.startswith("gemm_qkv")
    launch_args, checks, masks = [], [], {}
    for p in probs:
        kw = {k: v for k, v in p.items() if not isinstance(v, Spec)}
        t = {r: (_view(bufs[s.key], s) if r not in ("cos", "sin") else s.obj) for r, s in p.items() if isinstance(s, Spec)}
        Aspec, Wspec = p["A"], p["W"]
        batch, M = p.get("batch", 1), p["M"]
        Kd = Wspec.shape[-1] if qkv or p.get("K") is None else p["K"]      # (a QKV problem's "K" is the K output)
        N = (3 * p["H"] * 128) if qkv else (p.get("N") or Wspec.shape[-2])
        lda = p.get("lda") or Aspec.shape[-1]
        A3 = bufs[Aspec.key].as_strided((batch, M, Kd), (p.get("a_batch_stride", 0), lda, 1), Aspec.offset + p.get("a_offset", 0))
        W2 = bufs[Wspec.key].as_strided((N, Kd), (Wspec.stride[-2], 1), Wspec.offset)
        bias = t["bias"].reshape(-1)[:N] if "bias" in t else None
        if kind == "tagged":
            for z in range(batch):
                A3[z].copy_((A3[z].double() * R.tag_scales(M, Kd, z, device=DEV)).to(A3.dtype))
        chk = dict(qkv=qkv, A3=A3, W2=W2, bias=bias, M=M, N=N, batch=batch, p=p, t=t)
        if not qkv:
            out = p["out"]
            ldc = p.get("ldc") or N
            c_bs = p.get("c_batch_stride", 0)
            C3 = bufs[out.key].as_strided((batch, M, N), (c_bs, ldc, 1), out.offset + p.get("c_offset", 0))
            masks.setdefault(out.key, []).append(((batch, M, N), (c_bs, ldc, 1), out.offset + p.get("c_offset", 0)))
            chk["C3"] = C3
            if "out2" in t:
                chk["C2"] = bufs[p["out2"].key].as_strided((batch, M, N), (c_bs, ldc, 1), p["out2"].offset + p.get("c_offset", 0))
                masks.setdefault(p["out2"].key, []).append(((batch, M, N), (c_bs, ldc, 1), p["out2"].offset + p.get("c_offset", 0)))
            if "gate" in t:
                gs = p["gate"]
                chk["gate"] = bufs[gs.key].as_strided((batch, N), (p.get("gate_batch_stride", 0), 1), gs.offset)
            if "res" in t:
                rs = p["res"]
                res3 = bufs[rs.key].as_strided((batch, M, N), (p.get("res_batch_stride", 0), p.get("ldr") or ldc, 1), rs.offset + p.get("res_offset", 0))
                for z in range(batch):
                    for r0 in range(0, M, R.ROWS):
                        r1 = min(M, r0 + R.ROWS)
                        if kind == "cancel":       # res = -gate * lin: the output is the tiny rounding residual of res
                            lin, _ = R.linear_f64(A3[z, r0:r1], W2, bias)
                            gz = chk["gate"][z].double() if "gate" in chk else 1.0
                            res3[z, r0:r1] = (-gz * lin).to(res3.dtype)
                            del lin
                        else:
                            res3[z, r0:r1] = (R.lin_scale(Kd) * torch.randn((r1 - r0, N), device=DEV, generator=gen)).to(res3.dtype)
                chk["res"] = res3.clone()
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
            R.check_qkv(rep, c["A3"], c["W2"], c["bias"], t["norm_q"].reshape(-1)[:128], t["norm_k"].reshape(-1)[:128], t["cos"], t.get("sin"),
                        t["Q"], t["K"], t["VT"], H=p["H"], tok_off=p["tok_off"], rows_per_sample=p["rows_per_sample"],
                        q_scale=p.get("q_scale", 1.0), eps=p.get("eps", 1e-6), vt_perm=bool(p.get("vt_perm", False)))
        else:
            R.check_gemm(rep, c["A3"], c["W2"], c["bias"], c["C3"], act=p.get("act", 0), gate=c.get("gate"), res=c.get("res"),
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


def check_launch_list(rec):
    calls = rec["calls"]
    assert [c[0] for c in calls] == OPS, [c[0] for c in calls]
    D = 3072
    cp = dict(zip(LAUNCHES, [c[1] for c in calls]))
    assert cp["context_embedder"][0]["W"].shape == (D, 4096) and cp["context_embedder"][0]["M"] == rec["B"] * ST
    assert cp["x_embedder"][0]["W"].shape == (D, 64) and cp["x_embedder"][0]["c_offset"] == ST * D
    assert cp["proj_mlp"][0]["act"] == R.ACT_GELU_TANH and cp["proj_mlp"][0]["ldc"] == 5 * D and cp["proj_mlp"][0]["c_offset"] == D
    assert cp["single_proj_out"][0]["res"] is not None and cp["single_proj_out"][0]["gate"] is not None
    assert cp["final_proj_out"][0]["W"].shape == (64, D)
    for n in ("to_out_pair", "ff2_pair"):
        assert all(p.get("res") is not None and p.get("gate") is not None for p in cp[n])
    assert all(p.get("act") == R.ACT_GELU_TANH for p in cp["ff0_pair"])
    q = cp["qkv_pair"]
    assert (q[0]["tok_off"], q[0]["rows_per_sample"], q[1]["tok_off"], q[1]["rows_per_sample"]) == (ST, rec["Si"], 0, ST)
    assert cp["single_qkv"][0]["rows_per_sample"] == rec["S"] and cp["single_qkv"][0]["M"] == rec["B"] * rec["S"]


def run_config(ops, rec, kinds, label):
    t0 = time.time()
    seen = {}
    for kind in kinds:
        for i, name in enumerate(LAUNCHES):
            form, worst = replay(ops, rec, i, kind, seed=1000 * i + R.KINDS.index(kind))   # (new A, W, bias per kind)
            seen.setdefault(name, set()).add(form)
            WORST[name] = max(WORST.get(name, 0.0), worst)
    ops.streamk_check(sync=True)
    assert all(len(v) == 1 for v in seen.values()), seen
    got = {k: next(iter(v)) for k, v in seen.items()}
    print(f"\n  {label} ({time.time() - t0:.1f} s): forms {got}")
    print("  worst share of the f32 allowance: " + ", ".join(f"{k} {v:.3f}" for k, v in WORST.items()))
    return got


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_model_gemm_launches_vs_fp64(ops, cfg):
    rec = recording(ops, cfg)
    check_launch_list(rec)
    got = run_config(ops, rec, R.KINDS, cfg)
    assert got == DEFAULT_FORMS[cfg], (got, DEFAULT_FORMS[cfg])


@pytest.mark.parametrize("cfg,name,value,want", ALT_FORMS, ids=[f"{c}-{n}={v}" for c, n, v, _ in ALT_FORMS])
def test_alternative_kernel_forms_vs_fp64(ops, opt, cfg, name, value, want):
    rec = recording(ops, cfg)
    opt(name, value)
    got = run_config(ops, rec, R.KINDS, f"{cfg} {name}={value}")
    assert got == want, (got, want)
