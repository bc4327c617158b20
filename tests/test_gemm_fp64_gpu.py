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
from tests import gemm_replay as GR

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
# (Spec, the recorder, the operand fill and the replay itself live in tests/gemm_replay.py, shared with the encoder modules' test)
_recordings = {}


def recording(ops, cfg):
    """the named recording (gemm_replay.record) of one prepare_conditioning + denoise at configuration cfg, with the model's scalars"""
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

    def run():
        state = m.prepare_conditioning(enc, pooled, txt_ids.to(DEV), img_ids.reshape(-1, 3).to(DEV))
        m.denoise(state, hs, torch.full((B,), 0.75, device=DEV))
    calls = GR.record(ops, run)
    S = ST + Si
    rec = dict(calls=calls, names=LAUNCHES, B=B, Si=Si, S=S)
    del m
    _recordings.clear()
    _recordings[cfg] = rec
    return rec


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
            form, worst = GR.replay(ops, rec, name, kind, seed=1000 * i + R.KINDS.index(kind))   # (new A, W, bias per kind)
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
