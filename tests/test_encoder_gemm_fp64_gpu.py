"""Every bf16 GEMM launch of the encoder and decoder modules, at the modules' full widths, against the float64 reference of tests/gemm_ref.py
-- every output element of every launch, and the sentinel outside what the launch may write -- and the activation epilogues at toy shapes in
every kernel form.

T5, CLIP, the Qwen2 prefill (7B and 0.5B widths), the Qwen2.5-VL vision tower, SigLIP, the Resampler, Whisper, InternViT with its mlp1 tail, the
VAE mid-block attention and the projector heads push all their matrix work through ops.gemm, with geometry and epilogues the FLUX step of
tests/test_gemm_fp64_gpu.py never uses.  Each module is built at full width with ONE layer (two where only a layer that is not the last
makes a launch: the Qwen2 7B slab write, InternViT's in-place MLP branch) and random weights by the builders of its own stack test, runs
one forward under the recorder of tests/gemm_replay.py at the smallest row count that still reaches its row tiling, and every recorded
launch is replayed with each operand kind (gemm_ref.KINDS).  The launch list comes from the recording; what it must contain is asserted
per module, and so is the kernel form every launch took (last_gemm_tile; never 0, the generic form: every module promises K % 64 == 0
and the MFMA path).

Measured on MI355X (profiles/encoder_gemm_fp64_gputest.log): every launch and every grid case inside its bound, the worst share of the
f32 allowance 0.218 (InternViT proj: f32 layer scale with the residual in place); the module takes 20 s, of which T5's and the Qwen2
7B's weights on the host take 6 s and 5 s."""
import time

import pytest
import torch

from tests import gemm_ref as R
from tests import gemm_replay as GR

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
WORST = {}          # "module: launch" -> worst share of the f32 allowance used
WORST_ACT = {}      # activation name -> the same, over the toy grid


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


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------- what a recording holds
def launches(rec):
    """one dict per recorded ops.gemm problem: its geometry and what it uses"""
    out = []
    for (op, probs), name in zip(rec["calls"], rec["names"]):
        assert op == "gemm", (name, op)            # (no module here uses the pair or the fused-QKV entry points)
        p = probs[0]
        batch, M, N, K, lda, ldc = GR.geometry(p)
        res = p.get("res")
        out.append(dict(name=name, batch=batch, M=M, N=N, K=K, lda=lda, ldc=ldc, act=p.get("act", 0), bias=p.get("bias") is not None,
                        gate=p.get("gate") is not None, gate_f32=p.get("gate") is not None and p["gate"].dtype == torch.float32,
                        res=res is not None, inplace=res is not None and res.key == p["out"].key, ldr=p.get("ldr"),
                        a_off=p.get("a_offset", 0), c_off=p.get("c_offset", 0), c_bs=p.get("c_batch_stride", 0), a_bs=p.get("a_batch_stride", 0),
                        w_bs=p.get("w_batch_stride", 0), f32=bool(p.get("out_f32")), out2=p.get("out2") is not None, act2=p.get("act2", 0)))
    return out


def need(L, what, pred):
    hits = [l for l in L if pred(l)]
    assert hits, "the recording holds no %s; it holds %s" % (what, [l["name"] for l in L])
    return hits


# ---------------------------------------------------------------------------------------------------------------- the modules
# Each builder returns (run, check): run() is one forward of the module, check(L) asserts what launches(rec) must contain.
def build_t5():
    from tests import t5_ref as TR
    from x2i_amd.t5 import T5Stack
    d_model, heads, d_kv, d_ff, B, S = 4096, 64, 64, 10240, 2, 77
    cfg, lib = TR.library_stack(d_model, heads, d_kv, d_ff, 1)
    sd = TR.random_stack_state_dict(lib, seed=d_model + S)
    hip = T5Stack(cfg, device=DEV)
    hip.load_state_dict({k: v.bfloat16() for k, v in sd.items()}, strict=True)
    x = torch.randn((B, S, d_model), generator=gen(S)).bfloat16().to(DEV)

    def check(L):
        assert all(l["M"] == B * S for l in L)
        need(L, "qkv N=12288", lambda l: l["N"] == 12288 and l["K"] == 4096 and not l["bias"])
        need(L, "o with res in place", lambda l: l["N"] == 4096 and l["K"] == 4096 and l["inplace"])
        need(L, "fused wi N=20480", lambda l: l["N"] == 20480)
        need(L, "wo K=10240 with res in place", lambda l: l["K"] == 10240 and l["inplace"])
    return (lambda: hip(inputs_embeds=x)), check


def build_clip():
    from tests import clip_ref as CR
    from tests.test_clip_gpu import _lib_and_hip
    hidden, heads, inter, B, S = 768, 12, 3072, 2, 77
    _, _, hip = _lib_and_hip(hidden, heads, 1, inter, seed=hidden + S)
    ids = CR.ids_with_eos_at(B, S, 64, (S // 2, S - 1), 2, seed=S).to(DEV)

    def check(L):
        assert all(l["M"] == B * S for l in L)
        need(L, "qkv with bias", lambda l: l["N"] == 3 * hidden and l["bias"])
        need(L, "fc1", lambda l: l["N"] == inter and l["K"] == hidden and l["bias"] and not l["res"])
        need(L, "fc2 with res in place", lambda l: l["K"] == inter and l["inplace"])
        need(L, "out_proj with res in place", lambda l: l["K"] == hidden and l["N"] == hidden and l["inplace"])
    return (lambda: hip(ids, output_hidden_states=False)), check


def _build_qwen(hidden, Hq, Hkv, d_ff, layers, B, S, check):
    from tests import qwen_ref as QR
    from x2i_amd.qwen import Qwen2DecoderStack
    cfg, lib = QR.library_stack(hidden, Hq, Hkv, d_ff, layers)
    sd = QR.random_stack_state_dict(lib, seed=hidden + S)
    hip = Qwen2DecoderStack(cfg, device="cpu")
    hip.load_state_dict({k: v.bfloat16() for k, v in sd.items()}, strict=True)
    hip = hip.to(DEV)
    x = torch.randn((B, S, hidden), generator=gen(S)).bfloat16().to(DEV)
    return (lambda: hip(inputs_embeds=x)), check


def build_qwen_7b():
    B, S = 2, 130

    def check(L):
        need(L, "qkv N=4608 with bias", lambda l: l["N"] == 4608 and l["K"] == 3584 and l["bias"] and l["M"] == B * S)
        need(L, "batched o_proj", lambda l: l["batch"] == B and l["c_bs"] and l["N"] == 3584 and l["K"] == 3584 and l["M"] == S)
        need(L, "gu N=37888", lambda l: l["N"] == 37888 and l["K"] == 3584)
        need(L, "down K=18944 into the slab at c_offset", lambda l: l["K"] == 18944 and l["c_off"] and l["batch"] == B and l["res"])
    # (two layers: only a layer that is not the last writes its down projection into the slab, at the next entry's c_offset)
    return _build_qwen(3584, 28, 4, 18944, 2, B, S, check)


def build_qwen_05b():
    def check(L):
        assert all(l["M"] == 77 for l in L)
        need(L, "qkv N=1152", lambda l: l["N"] == 1152 and l["K"] == 896 and l["bias"])
        need(L, "down K=4864", lambda l: l["K"] == 4864)
    return _build_qwen(896, 14, 2, 4864, 1, 1, 77, check)


def build_qwen_vision():
    from tests import qwen_vision_ref as VR
    from x2i_amd.qwen_vision import Qwen2_5VisionTower
    hidden, heads, inter, out_hidden, grid = 1280, 16, 3420, 3584, [(1, 10, 10)]
    cfg, lib = VR.library_tower(1, hidden, heads, inter, out_hidden, (0,))
    sd = VR.random_tower_state_dict(lib, seed=hidden + len(grid))
    hip = Qwen2_5VisionTower(cfg, device="cpu")
    hip.load_state_dict({k: v.bfloat16() for k, v in sd.items()}, strict=True)
    hip = hip.to(DEV)
    px, g = VR.pixel_rows(grid, seed=hidden).to(DEV), torch.tensor(grid)
    plan = hip.plan(g)

    def check(L):
        need(L, "pe K=1216", lambda l: l["K"] == 1216 and l["N"] == hidden and l["M"] == 100)
        need(L, "gu N=6912", lambda l: l["N"] == 6912 and l["M"] == 100)
        need(L, "down K=3456 with res, ldr", lambda l: l["K"] == 3456 and l["res"] and not l["inplace"] and l["ldr"] == hidden)
        need(L, "proj with res, ldr", lambda l: l["K"] == hidden and l["N"] == hidden and l["res"] and l["ldr"] == hidden)
        need(L, "merger fc1 with GELU-erf at M=25", lambda l: l["M"] == 25 and l["K"] == 4 * hidden and l["act"] == R.ACT_GELU_ERF)
        need(L, "merger fc2", lambda l: l["M"] == 25 and l["N"] == out_hidden)
    return (lambda: hip(px, plan=plan)), check


def build_siglip():
    from tests import siglip_ref as SR
    from x2i_amd.siglip import SiglipVisionTower
    hidden, heads, inter, grids = 1152, 16, 4304, [(32, 32), (20, 27)]
    cfg, lib = SR.library_tower(hidden, heads, inter, 1)
    sd = SR.random_state_dict(lib, seed=hidden + len(grids))
    hip = SiglipVisionTower(cfg, device="cpu")
    hip.load_state_dict({k: v.bfloat16() for k, v in sd.items()}, strict=True)
    hip = hip.to(DEV)
    L_ = max(h * w for h, w in grids)
    strips, _ = SR.random_strips(grids, L_, seed=hidden)
    x = strips.bfloat16().to(DEV)
    plan = hip.plan(grids, L_)

    def check(L):
        assert all(l["M"] == len(grids) * L_ for l in L)
        need(L, "pe K=640", lambda l: l["K"] == 640 and l["N"] == hidden)
        need(L, "qkv N=3840 (heads of 72 padded to 80)", lambda l: l["N"] == 3840 and l["K"] == hidden)
        need(L, "out_proj K=1280 with res in place", lambda l: l["K"] == 1280 and l["inplace"])
        need(L, "fc1 N=4352 with GELU-tanh", lambda l: l["N"] == 4352 and l["act"] == R.ACT_GELU_TANH)
        need(L, "fc2 K=4352 with res in place", lambda l: l["K"] == 4352 and l["inplace"])
    return (lambda: hip(x, plan=plan)), check


def build_resampler(frames=None):
    """frames None: the stack test's full-width case, two frames in one chunk.  frames = 17 small ones: a second chunk of the 16-frame
    chunking, whose kv_proj reads x at a_offset and whose projT writes at c_offset"""
    from tests import resampler_ref as RR
    from tests.test_resampler_gpu import MODULE_CASES, hip_module
    D, kv, NQ, grids = MODULE_CASES[-1]
    assert (D, kv, NQ) == (3584, 1152, 64)
    if frames:
        grids = [(2, 3)] * frames
    hip = hip_module(RR.random_state_dict(NQ, D, kv, seed=D + kv), NQ, D, kv)
    L_ = max(h * w for h, w in grids)
    x = RR.random_input(grids, L_, kv, seed=D).bfloat16().to(DEV)
    sizes = torch.tensor(grids, dtype=torch.int32, device=DEV)

    def check(L):
        need(L, "kv_proj K=1152", lambda l: l["K"] == kv and l["N"] == D and not l["bias"])
        if frames:
            need(L, "kv_proj read at a_offset", lambda l: l["K"] == kv and l["a_off"] == 16 * L_ * kv and l["M"] == (frames - 16) * L_)
            need(L, "projT written at c_offset", lambda l: not l["bias"] and l["c_off"] == 16 * NQ * D and l["M"] == (frames - 16) * NQ)
        need(L, "K into [M, 2D] by ldc", lambda l: l["ldc"] == 2 * D and l["N"] == D and not l["c_off"])
        need(L, "V into [M, 2D] by ldc at c_offset", lambda l: l["ldc"] == 2 * D and l["N"] == D and l["c_off"] == D)
        need(L, "out_proj", lambda l: l["M"] == min(len(grids), 16) * NQ and l["bias"] and l["N"] == D)
        need(L, "projT", lambda l: l["M"] == min(len(grids), 16) * NQ and not l["bias"] and l["N"] == D and l["ldc"] == D)
    return (lambda: hip(x, sizes)), check


def _build_whisper(T, lens):
    """T mel frames.  The plan (x2i_amd/whisper.py: plan) accepts every T >= 1; S = conv_rows(T) = (T - 1) // 2 + 1 rows leave the stem and
    n = pooled_rows(S, 2) leave the pool, and the projection launches only where n >= 1, that is S >= 2: T = 3 is the shortest length at
    which the forward makes every one of its launches.  T = 260 (S = 130) is the stack test's padded batch: rows past one 128-row tile, and
    130 overlapping A rows in conv2."""
    from tests import whisper_ref as WR
    from x2i_amd.whisper import WhisperAudioTower
    D, heads, ffn, E, k = 1024, 16, 4096, 3584, 2
    cfg, apm, proj = WR.library_tower(D, heads, ffn, 1, 1500, E)
    WR.load_state_dict_into(apm, proj, WR.random_state_dict(apm, proj, seed=D + T))
    hip = WhisperAudioTower.from_hf(apm, proj, k).to(DEV)
    B = len(lens)
    x = WR.random_mel(B, T, lens, seed=T).bfloat16().to(DEV)
    plan = hip.plan(lens, T, 50)
    S = (T - 1) // 2 + 1

    def check(L):
        need(L, "conv1 batched with c_offset and GELU-erf",
             lambda l: l["batch"] == B and l["M"] == T and l["c_off"] == D and l["act"] == R.ACT_GELU_ERF)
        need(L, "conv2 with lda = 2D, K = 3D", lambda l: l["lda"] == 2 * D and l["K"] == 3 * D and l["M"] == S and l["act"] == R.ACT_GELU_ERF)
        need(L, "fc1 with GELU-erf", lambda l: l["N"] == ffn and l["act"] == R.ACT_GELU_ERF and l["M"] == B * S)
        need(L, "fc2 with res in place", lambda l: l["K"] == ffn and l["inplace"])
        need(L, "projection with ReLU", lambda l: l["N"] == E and l["K"] == D and l["act"] == R.ACT_RELU)
        need(L, "projection linear2", lambda l: l["N"] == E and l["K"] == E and l["M"] == B * (S // k))
    return (lambda: hip(x, plan=plan)), check


def build_internvit():
    from tests import internvit_ref as IR
    from tests.test_internvit_gpu import FULL, _hip_vision
    cfg, llm, B = FULL, 896, 2           # (two layers, as the stack test: only a layer that is not the last adds its MLP branch in place)
    assert (cfg["hidden_size"], cfg["num_attention_heads"], cfg["intermediate_size"]) == (1024, 16, 4096)
    vis = _hip_vision(IR.random_state_dict(cfg, llm, seed=cfg["hidden_size"] + B), cfg, llm)
    px = IR.random_pixels(B, cfg["image_size"], seed=cfg["hidden_size"]).bfloat16().to(DEV)
    g = cfg["image_size"] // cfg["patch_size"]
    plan = vis.plan(B, g)

    def check(L):
        need(L, "batched pe with c_offset", lambda l: l["batch"] == B and l["M"] == g * g and l["c_off"] == 1024 and l["N"] == 1024)
        need(L, "qkv at M = 2 x 1025", lambda l: l["M"] == B * 1025 and l["N"] == 3072)
        need(L, "proj with f32 gate and res in place", lambda l: l["K"] == 1024 and l["N"] == 1024 and l["gate_f32"] and l["inplace"])
        need(L, "fc1 with GELU-erf", lambda l: l["N"] == 4096 and l["K"] == 1024 and l["act"] == R.ACT_GELU_ERF)
        need(L, "fc2 with f32 gate and res in place", lambda l: l["K"] == 4096 and l["N"] == 1024 and l["gate_f32"] and l["inplace"])
        need(L, "the last fc2, with f32 gate and res, into the output", lambda l: l["K"] == 4096 and l["gate_f32"] and l["res"] and not l["inplace"])
        need(L, "mlp1 GELU-erf at K=4096", lambda l: l["K"] == 4096 and l["N"] == llm and l["act"] == R.ACT_GELU_ERF)
        need(L, "mlp1 second linear", lambda l: l["K"] == llm and l["N"] == llm)
    return (lambda: vis(px, plan=plan)), check


def build_vae_attention():
    from x2i_amd.vae import AutoencoderKL
    B, C, h = 2, 512, 16
    vae = AutoencoderKL(device=DEV).init_random_(seed=7)
    attn = vae.decoder.mid_block.attentions[0]
    assert attn.c == C
    x = torch.randn((B, h, h, C), generator=gen(8)).bfloat16().to(DEV)
    T = h * h

    def check(L):
        wb = need(L, "launch with w_batch_stride", lambda l: l["w_bs"])
        assert len(wb) == 3 and all(l["batch"] == B for l in wb), [l["name"] for l in wb]
        need(L, "V^T: h as the weight, one shared A", lambda l: l["w_bs"] == T * C and l["a_bs"] == 0 and l["M"] == C and l["N"] == T)
        need(L, "scores: k as the weight", lambda l: l["w_bs"] == T * C and l["a_bs"] == T * C and l["M"] == T and l["N"] == T)
        need(L, "P V: V^T as the weight", lambda l: l["w_bs"] == C * T and l["K"] == T and l["N"] == C and l["bias"])
        need(L, "to_out with res, ldr", lambda l: l["M"] == B * T and l["res"] and not l["inplace"] and l["ldr"] == C)
    return (lambda: attn.run(x, h, h, vae.config.norm_num_groups)), check


def build_proj_heads():
    """The InternVL-1B head (tests/test_proj_fp64_gpu.py's width H = 896, and its smallest B x S at that width: 2 x 40) and, for the
    act-only chain, a legacy head of the same widths"""
    import x2i_amd.proj as XP
    B, C, S, H = 2, 29, 40, 896
    head = XP.create_proj_internvl1b(C, use_t5=False, use_scale=True, device=DEV).init_random_(seed=3)
    x = torch.randn((B, C, S, H), generator=gen(4)).bfloat16().to(DEV)

    def check(L):
        assert all(l["M"] == B * S for l in L)
        need(L, "act-only launch (GELU-erf, no bias)", lambda l: l["act"] == R.ACT_GELU_ERF and not l["bias"] and not l["out2"] and l["K"] == H)
        need(L, "out2 + act2 GELU-erf", lambda l: l["out2"] and l["act2"] == R.ACT_GELU_ERF and l["act"] == 0)
        need(L, "out_f32", lambda l: l["f32"] and l["bias"] and l["N"] == 768)
    return (lambda: head(x)), check


MODULES = {"t5": build_t5, "clip": build_clip, "qwen2_7b": build_qwen_7b, "qwen2_05b": build_qwen_05b, "qwen_vision": build_qwen_vision,
           "siglip": build_siglip, "resampler": build_resampler, "resampler_17_frames": lambda: build_resampler(17),
           "whisper_t3": lambda: _build_whisper(3, [3, 3]),
           "whisper_t260": lambda: _build_whisper(260, [260, 90]), "internvit": build_internvit, "vae_attention": build_vae_attention,
           "proj_heads": build_proj_heads}

# the kernel form of every launch (last_gemm_tile after the call), measured on MI355X; the names are gemm_replay.describe()'s: the launch's
# place in the forward, batch x M x N x K and what it uses
FORMS = {
    "t5": {'00 154x12288x4096': 128, '01 154x4096x4096 res_inplace': 128, '02 154x20480x4096': 128, '03 154x4096x10240 res_inplace': 128},
    "clip": {'00 154x2304x768 bias': 128, '01 154x768x768 bias res_inplace': 128, '02 154x3072x768 bias': 128,
        '03 154x768x3072 bias res_inplace': 128},
    "qwen2_7b": {'00 260x4608x3584 bias': 128, '01 2x130x3584x3584 res ldr': 128, '02 260x37888x3584': 128,
        '03 2x130x3584x18944 res ldr c_off': 128, '04 260x4608x3584 bias': 128, '05 2x130x3584x3584 res ldr': 128, '06 260x37888x3584': 128,
        '07 260x3584x18944 res ldr': 128},
    "qwen2_05b": {'00 77x1152x896 bias': 128, '01 77x896x896 res ldr': 128, '02 77x9728x896': 128, '03 77x896x4864 res ldr': 128},
    "qwen_vision": {'00 100x1280x1216': 128, '01 100x3840x1280 bias': 128, '02 100x1280x1280 bias res ldr': 128, '03 100x6912x1280 bias': 128,
        '04 100x1280x3456 bias res ldr': 128, '05 25x5120x5120 gelu_erf bias': 128, '06 25x3584x5120 bias': 128},
    "siglip": {'00 2048x1152x640 bias': 128, '01 2048x3840x1152 bias': 128, '02 2048x1152x1280 bias res_inplace': 128,
        '03 2048x4352x1152 gelu_tanh bias': 256, '04 2048x1152x4352 bias res_inplace': 128},
    "resampler": {'00 64x3584x3584 bias': 128, '01 2048x3584x1152': 128, '02 2048x3584x3584 bias ldc7168': 128,
        '03 2048x3584x3584 bias c_off ldc7168': 128, '04 128x3584x3584 bias': 128, '05 128x3584x3584': 128},
    "resampler_17_frames": {'00 64x3584x3584 bias': 128, '01 96x3584x1152': 128, '02 96x3584x3584 bias ldc7168': 128,
        '03 96x3584x3584 bias c_off ldc7168': 128, '04 1024x3584x3584 bias': 128, '05 1024x3584x3584': 128, '06 6x3584x1152 a_off': 128,
        '07 6x3584x3584 bias ldc7168': 128, '08 6x3584x3584 bias c_off ldc7168': 128, '09 64x3584x3584 bias': 128, '10 64x3584x3584 c_off': 128},
    "whisper_t3": {'00 2x3x1024x256 gelu_erf bias c_off': 128, '01 2x2x1024x3072 gelu_erf bias lda2048': 128, '02 4x3072x1024 bias': 128,
        '03 4x1024x1024 bias res_inplace': 128, '04 4x4096x1024 gelu_erf bias': 128, '05 4x1024x4096 bias res_inplace': 128,
        '06 4x3584x1024 relu bias': 128, '07 2x3584x3584 bias': 128},
    "whisper_t260": {'00 2x260x1024x256 gelu_erf bias c_off': 128, '01 2x130x1024x3072 gelu_erf bias lda2048': 128, '02 260x3072x1024 bias': 128,
        '03 260x1024x1024 bias res_inplace': 128, '04 260x4096x1024 gelu_erf bias': 128, '05 260x1024x4096 bias res_inplace': 128,
        '06 260x3584x1024 relu bias': 128, '07 130x3584x3584 bias': 128},
    "internvit": {'00 2x1024x1024x640 bias c_off': 128, '01 2050x3072x1024 bias': 128, '02 2050x1024x1024 bias gate res_inplace': 128,
        '03 2050x4096x1024 gelu_erf bias': 256, '04 2050x1024x4096 bias gate res_inplace': 128, '05 2050x3072x1024 bias': 128,
        '06 2050x1024x1024 bias gate res_inplace': 128, '07 2050x4096x1024 gelu_erf bias': 256, '08 2050x1024x4096 bias gate res': 128,
        '09 512x896x4096 gelu_erf bias': 128, '10 512x896x896 bias': 128},
    "vae_attention": {'00 512x512x512 bias': 128, '01 512x512x512 bias': 128, '02 2x512x256x512 wbatch shared_a': 128,
        '03 2x256x256x512 wbatch': 128, '04 2x256x512x256 bias wbatch': 128, '05 512x512x512 bias res ldr': 128},
    "proj_heads": {'00 80x4096x896 gelu_erf': 128, '01 80x4096x4096 out2_gelu_erf': 128, '02 80x768x4096 bias f32': 128},
}


def run_module(ops, rec, label):
    t0 = time.time()
    got = {}
    for i, name in enumerate(rec["names"]):
        forms, worst = set(), 0.0
        for kind in R.KINDS:
            form, w = GR.replay(ops, rec, name, kind, seed=1000 * i + R.KINDS.index(kind))
            forms.add(form)
            worst = max(worst, w)
        assert len(forms) == 1, (name, forms)
        got[name] = forms.pop()
        WORST["%s: %s" % (label, name)] = worst
    ops.streamk_check(sync=True)
    print(f"\n  {label} ({time.time() - t0:.1f} s replaying {len(got)} launches x {len(R.KINDS)} kinds)")
    for name, form in got.items():
        print(f"    {label}: {name!r}: {form},    # share {WORST['%s: %s' % (label, name)]:.3f}")
    return got


@pytest.mark.parametrize("module", list(MODULES))
def test_module_gemm_launches_vs_fp64(ops, module):
    t0 = time.time()
    run, check = MODULES[module]()
    rec = GR.named(GR.record(ops, run))
    check(launches(rec))
    print(f"\n  {module}: built and recorded in {time.time() - t0:.1f} s")
    del run, check
    got = run_module(ops, rec, module)
    assert all(form != 0 for form in got.values()), "a full-width launch took the generic form: %s" % got
    assert got == FORMS.get(module), (got, FORMS.get(module))


# ---------------------------------------------------------------------------------------------------------------- epilogue grid
# (M, N, K, gemm_tile): ragged in both tile sizes, more than one block; K = 27 (no multiple of 64) takes the generic form
GRID = {"mfma_tile128": (130, 200, 192, 128), "mfma_tile256": (130, 200, 192, 256), "generic": (37, 50, 27, None)}
# ("none": the f32 output and the gated in-place residual on the MFMA forms too -- with an activation the launcher has no MFMA kernel for them)
ACTS = {"none": R.ACT_NONE, "gelu_tanh": R.ACT_GELU_TANH, "gelu_erf": R.ACT_GELU_ERF, "silu": R.ACT_SILU, "relu": R.ACT_RELU}
VARIANTS = ("plain", "out_f32", "out2", "gate_res_inplace", "ldc_slab")
MARGIN = 8          # sentinel elements behind every output row


def grid_forms(shape, act):
    """The form every variant takes, measured on MI355X: the forced tile's kernel, except that the MFMA kernels are not instantiated for an
    activation together with an f32 output or with a residual (csrc/gemm.hip: plan_gemm): those two go to the generic kernel at this size
    (and are refused at a size too large for it)."""
    tile = GRID[shape][3] or 0
    return {v: (0 if act != "none" and v in ("out_f32", "gate_res_inplace") else tile) for v in VARIANTS}


def grid_case(ops, shape, act, variant, kind, seed):
    """one launch of the grid; returns (form, share of the f32 allowance)"""
    from x2i_amd import _lib
    M, N, K, _ = GRID[shape]
    g = torch.Generator(device=DEV).manual_seed(seed)
    A = 3.0 * torch.randn((M, K), device=DEV, generator=g)                 # lin reaches the activations' tails on both sides
    if kind == "tagged":
        A = A * R.tag_scales(M, K, device=DEV)
    A = A.to(BF)
    W = (0.1 * torch.randn((N, K), device=DEV, generator=g)).to(BF)
    bias = (0.5 * torch.randn((N,), device=DEV, generator=g)).to(BF)
    ldc, c_off = (2 * N + 2 * MARGIN, N + MARGIN) if variant == "ldc_slab" else (N + MARGIN, 0)
    f32 = variant == "out_f32"
    buf = R.poison_(torch.empty(M * ldc + 3, device=DEV, dtype=torch.float32 if f32 else BF))
    view = ((M, N), (ldc, 1), c_off)
    kw = dict(out=buf, M=M, ldc=ldc, c_offset=c_off, out_f32=f32)
    exp = dict(out_f32=f32)
    buf2 = None
    if variant == "out2":
        buf2 = R.poison_(torch.empty_like(buf))
        kw.update(out2=buf2, act2=act)
        exp.update(act2=act)
    else:
        kw.update(act=act)
        exp.update(act=act)
    if variant == "gate_res_inplace":
        gate = torch.randn((N,), device=DEV, generator=g)
        lin, _ = R.linear_f64(A, W, bias)
        if kind == "cancel":
            resv = (-gate.double() * R.act_f64(lin, act)).to(BF)
        else:
            resv = (float(lin.std()) * torch.randn((M, N), device=DEV, generator=g)).to(BF)
        buf.as_strided(*view).copy_(resv)                                   # the residual lives in the output's storage
        kw.update(res=buf, gate=gate, ldr=ldc)
        exp.update(res=resv, gate=gate)
    ops.gemm(A, W, bias, **kw)
    form = int(_lib.get_option("last_gemm_tile"))
    torch.cuda.synchronize()
    name = f"grid {shape} {act} {variant} {kind}"
    e = R.gemm_expect(A, W, bias, **exp)
    (want, bound, d), e2 = (e if variant == "out2" else (e, None))
    msg, share, _, _ = R.check_block(name, buf.as_strided(*view), want, bound, delta=d)
    assert msg is None, msg
    R.check_untouched(name, buf, R.write_mask(buf, [view]), row_len=ldc)
    if e2 is not None:
        msg, share2, _, _ = R.check_block(name + " C2", buf2.as_strided(*view), e2[0], e2[1], delta=e2[2])
        assert msg is None, msg
        R.check_untouched(name + " C2", buf2, R.write_mask(buf2, [view]), row_len=ldc)
        share = max(share, share2)
    return form, share


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("shape", list(GRID))
def test_epilogue_grid_vs_fp64(ops, opt, shape, act):
    from x2i_amd._lib import X2IError
    tile = GRID[shape][3]
    if tile is not None:
        opt("gemm_tile", tile)
    got, line = {}, []
    for vi, variant in enumerate(VARIANTS):
        worst, forms = 0.0, set()
        for ki, kind in enumerate(R.KINDS):
            try:
                form, share = grid_case(ops, shape, ACTS[act], variant, kind, seed=100 * vi + 10 * ki + ACTS[act])
            except X2IError as e:
                assert shape == "generic", (shape, act, variant, str(e))    # the generic form runs what the launcher accepts for it
                line.append(f"{variant} refused")
                break
            forms.add(form)
            worst = max(worst, share)
        else:
            assert len(forms) == 1, (variant, forms)
            got[variant] = forms.pop()
            line.append(f"{variant} {worst:.3f}")
            WORST_ACT[act] = max(WORST_ACT.get(act, 0.0), worst)
    print(f"\n  grid {shape} {act}: forms {got}; share of the f32 allowance: " + ", ".join(line))
    assert got == grid_forms(shape, act), (got, grid_forms(shape, act))


def test_print_worst():
    """(last: the table of the run)"""
    print("\n  worst share of the f32 allowance per launch:")
    for k, v in WORST.items():
        print(f"    {k}: {v:.3f}")
    print("  per activation over the toy grid: " + ", ".join(f"{k} {v:.3f}" for k, v in WORST_ACT.items()))
