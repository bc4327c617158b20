"""References and helpers for the InternVL2.5 vision path's kernels and host modules (include/x2i_internvit.h, x2i_amd/internvit.py).
No GPU-only code here: the CPU tests import it too.

  tower, tail   InternVisionModel and the tail of extract_feature (class token dropped, pixel_shuffle(0.5), mlp1) restated from torch.nn
                pieces, parametrised by dtype.  In float64 it is the judge; in bf16 every operation rounds where the model's own bf16 run
                rounds (the Conv2d, the cat and the position add, each norm, each linear, q * scale, the scores, the softmax, the
                context, the GELU, the LayerScale product, the residual sum), so it is the comparator: the library's own bf16 error.
  faults        the same restatement with one planted fault, for the test that the criterion of the GPU test rejects each of them
  checker       check_extract_feature: relative L2 error against float64 no worse than 1.5 x the bf16 restatement's and below 3e-2 (the
                criterion of tests/test_siglip_gpu.py), on the test weights and on a second set that makes the form of the GELU visible
"""
import torch
import torch.nn.functional as F

from tests.t5_ref import rel_l2  # noqa: F401  (for the tests that import this module)

FAULTS = ("chunks_swapped", "v1_for_v2", "class_row_kept", "ls_omitted", "gelu_tanh", "scale_of_wrong_width")

TINY = dict(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=256, image_size=56, patch_size=14,
            layer_norm_eps=1e-6, hidden_act="gelu", norm_type="layer_norm", qk_normalization=False, qkv_bias=True)
TINY_LLM = 192


# ---------------------------------------------------------------------------------------------------------------- weights and inputs
def state_dict_shapes(cfg, llm=None):
    """{name: shape} of InternVisionModel's state dict for the configuration cfg (the reference's parameter names); with llm, the chat
    model's `vision_model.` prefix and its mlp1 as well"""
    D, F_, P, N = cfg["hidden_size"], cfg["intermediate_size"], cfg["patch_size"], (cfg["image_size"] // cfg["patch_size"]) ** 2
    s = {"embeddings.class_embedding": (1, 1, D), "embeddings.patch_embedding.weight": (D, 3, P, P), "embeddings.patch_embedding.bias": (D,),
         "embeddings.position_embedding": (1, N + 1, D)}
    for i in range(cfg["num_hidden_layers"]):
        p = "encoder.layers.%d." % i
        s[p + "attn.qkv.weight"] = (3 * D, D)
        if cfg.get("qkv_bias", True):
            s[p + "attn.qkv.bias"] = (3 * D,)
        if cfg.get("qk_normalization", False):
            s[p + "attn.q_norm.weight"] = (D,)
            s[p + "attn.k_norm.weight"] = (D,)
        s.update({p + "attn.proj.weight": (D, D), p + "attn.proj.bias": (D,), p + "mlp.fc1.weight": (F_, D), p + "mlp.fc1.bias": (F_,),
                  p + "mlp.fc2.weight": (D, F_), p + "mlp.fc2.bias": (D,), p + "norm1.weight": (D,), p + "norm2.weight": (D,),
                  p + "ls1": (D,), p + "ls2": (D,)})
        if cfg.get("norm_type", "layer_norm") == "layer_norm":
            s.update({p + "norm1.bias": (D,), p + "norm2.bias": (D,)})
    if llm is None:
        return s
    s = {"vision_model." + k: v for k, v in s.items()}
    s.update({"mlp1.0.weight": (4 * D,), "mlp1.0.bias": (4 * D,), "mlp1.1.weight": (llm, 4 * D), "mlp1.1.bias": (llm,),
              "mlp1.3.weight": (llm, llm), "mlp1.3.bias": (llm,)})
    return s


def random_state_dict(cfg, llm, seed):
    """The test weights: matrices (the Conv2d kernel included) N(0, 1 / fan_in); the class token and the position table N(0, 0.02^2) -- the
    checkpoint's scale, not the constructor's N(0, 1); norm weights 1 + 0.1 N(0, 1) and biases 0.1 N(0, 1), whose defaults would hide a
    missing one; ls1 / ls2 0.1 (1 + 0.5 N(0, 1)), NOT the constructor's 0.1 everywhere; float32 tensors that hold bf16 values"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in state_dict_shapes(cfg, llm).items():
        r = torch.randn(shape, generator=g)
        if k.endswith("class_embedding") or k.endswith("position_embedding"):
            v = 0.02 * r
        elif k.endswith("ls1") or k.endswith("ls2"):
            v = 0.1 * (1.0 + 0.5 * r)
        elif len(shape) == 1:
            v = (1.0 if ("norm" in k or k == "mlp1.0.weight") and k.endswith("weight") else 0.0) + 0.1 * r
        else:
            v = r * (r.numel() // shape[0]) ** -0.5
        sd[k] = v.bfloat16().float()
    return sd


def fixture_state_dict(cfg, llm, seed):
    """random_state_dict with every matrix snapped to 127 steps of a power of two per tensor: still bf16 values (seven bits and a sign
    times a power of two), and one byte per weight in the fixture (pack_state_dict) where bf16 takes two -- the matrices are nine tenths
    of the fixture"""
    sd = random_state_dict(cfg, llm, seed)
    for k, v in sd.items():
        if v.dim() >= 2 and v.numel() > 4096:
            step = 2.0 ** torch.ceil(torch.log2(v.abs().max() / 127.0))
            sd[k] = torch.round(v / step).clamp(-127, 127) * step
            assert torch.equal(sd[k].bfloat16().float(), sd[k])
    return sd


def pack_state_dict(sd):
    """{'sd.' + name: bf16 tensor} for the small tensors, {'q.' + name: int8, 'step.' + name: f32 scalar} for fixture_state_dict's matrices"""
    out = {}
    for k, v in sd.items():
        if v.dim() >= 2 and v.numel() > 4096:
            step = 2.0 ** torch.ceil(torch.log2(v.abs().max() / 127.0))
            q = torch.round(v / step)
            assert torch.equal(q * step, v) and float(q.abs().max()) <= 127, k
            out["q." + k], out["step." + k] = q.to(torch.int8).contiguous(), step.reshape(1).float()
        else:
            assert torch.equal(v.bfloat16().float(), v), k
            out["sd." + k] = v.bfloat16().contiguous()
    return out


def unpack_state_dict(tensors):
    """The float32 state dict of a fixture written with pack_state_dict"""
    sd = {k[3:]: v.float() for k, v in tensors.items() if k.startswith("sd.")}
    sd.update({k[2:]: v.float() * tensors["step." + k[2:]].float() for k, v in tensors.items() if k.startswith("q.")})
    return sd


def random_pixels(B, side, seed):
    """[B, 3, side, side] of N(0, 1) pixels holding bf16 values"""
    return torch.randn((B, 3, side, side), generator=torch.Generator().manual_seed(seed)).bfloat16().float()


# ---------------------------------------------------------------------------------------------------------------- pieces
def patch_rows(img, P, Kp=None):
    """[B, 3, gh*P, gw*P] -> [B*gh*gw, 3*P*P] in the Conv2d weight's column order (row b*L + r*gw + q), with a zero tail up to Kp"""
    B, _, Hh, Ww = img.shape
    gh, gw = Hh // P, Ww // P
    rows = img.reshape(B, 3, gh, P, gw, P).permute(0, 2, 4, 1, 3, 5).reshape(B * gh * gw, 3 * P * P)
    if Kp is None:
        return rows
    return torch.cat((rows, torch.zeros((rows.shape[0], Kp - 3 * P * P), dtype=img.dtype, device=img.device)), 1)


def position_table(pos, side, gh, gw):
    """[1, 1 + gh*gw, D] in pos's dtype: the class row, then the patch rows of pos [1, 1 + side*side, D] resampled to gh x gw in float32
    (bicubic, align_corners=False) on the CPU and cast back: the model's own call"""
    grid = pos[:, 1:, :].detach().cpu().float().reshape(1, side, side, -1).permute(0, 3, 1, 2)
    grid = F.interpolate(grid, size=(gh, gw), mode="bicubic", align_corners=False).reshape(1, -1, gh * gw).permute(0, 2, 1)
    return torch.cat([pos[:, :1, :], grid.to(device=pos.device, dtype=pos.dtype)], dim=1)


def shuffle_gather(tokens, g, v1=False, swap=False):
    """pixel_shuffle(0.5) of tokens [B, g*g, D] (no class row) as one index expression -> [B, (g/2)^2, 4*D]: row t = r' g/2 + q' (v2) or
    q' g/2 + r' (v1) holds the tokens (2r' + dr, 2q' + dq) for (dr, dq) = (0,0), (0,1), (1,0), (1,1).  swap: the planted fault, the
    chunks (0,1) and (1,0) exchanged"""
    B, _, D = tokens.shape
    x = tokens.reshape(B, g // 2, 2, g // 2, 2, D)      # [b, r', dr, q', dq, d]
    x = x.permute(0, 3, 1, 2, 4, 5) if v1 else x.permute(0, 1, 3, 2, 4, 5)      # [b, t, dr, dq, d] with t over two axes
    if swap:
        x = x.transpose(3, 4)
    return x.reshape(B, (g // 2) ** 2, 4 * D)


def _rms(x, w, eps):
    """InternRMSNorm: float32 statistics (float64 under float64), the normalised value cast back BEFORE the weight multiplies it"""
    h = x.to(torch.float64 if x.dtype == torch.float64 else torch.float32)
    h = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + eps)
    return w * h.to(x.dtype)


# ---------------------------------------------------------------------------------------------------------------- the tower and the tail
def tower(sd, pixels, cfg, dtype, select_layer=-1, attn="naive", fault=None, prefix="", pos=None):
    """hidden_states[select_layer] of InternVisionModel, [B, 1 + gh*gw, D] in `dtype`, from the state dict sd (the reference's names behind
    `prefix`) on the device of `pixels`.  attn: 'naive' (the reference without flash attention: the scores materialised) or 'sdpa'.
    pos: the grid's position table made earlier (position_table), for a timed loop that should not go through the CPU every call."""
    dev = pixels.device
    w = lambda k: sd[prefix + k].to(device=dev, dtype=dtype)
    D, H, P, eps = cfg["hidden_size"], cfg["num_attention_heads"], cfg["patch_size"], cfg["layer_norm_eps"]
    NL, side, dk = cfg["num_hidden_layers"], cfg["image_size"] // cfg["patch_size"], cfg["hidden_size"] // cfg["num_attention_heads"]
    rms = cfg.get("norm_type", "layer_norm") == "rms_norm"
    x = pixels.to(dtype)
    B, gh, gw = x.shape[0], x.shape[2] // P, x.shape[3] // P
    pe = F.conv2d(x, w("embeddings.patch_embedding.weight"), w("embeddings.patch_embedding.bias"), stride=P).flatten(2).transpose(1, 2)
    x = torch.cat([w("embeddings.class_embedding").expand(B, 1, -1), pe], dim=1)
    x = x + (position_table(w("embeddings.position_embedding"), side, gh, gw) if pos is None else pos)
    scale = (2 * dk if fault == "scale_of_wrong_width" else dk) ** -0.5
    act = (lambda t: F.gelu(t, approximate="tanh")) if fault == "gelu_tanh" else F.gelu
    n_run = select_layer if select_layer >= 0 else NL + 1 + select_layer
    assert 0 <= n_run <= NL
    for i in range(n_run):
        p = "encoder.layers.%d." % i
        norm = (lambda t, nm: _rms(t, w(p + nm + ".weight"), eps)) if rms else \
               (lambda t, nm: F.layer_norm(t, (D,), w(p + nm + ".weight"), w(p + nm + ".bias"), eps))
        lin = lambda t, nm: F.linear(t, w(p + nm + ".weight"), w(p + nm + ".bias") if prefix + p + nm + ".bias" in sd else None)
        S = x.shape[1]
        qkv = lin(norm(x, "norm1"), "attn.qkv").reshape(B, S, 3, H, dk).permute(2, 0, 3, 1, 4)
        q, k, v = qkv.unbind(0)
        if cfg.get("qk_normalization", False):
            q = _rms(q.transpose(1, 2).flatten(-2, -1), w(p + "attn.q_norm.weight"), eps).view(B, S, H, dk).transpose(1, 2)
            k = _rms(k.transpose(1, 2).flatten(-2, -1), w(p + "attn.k_norm.weight"), eps).view(B, S, H, dk).transpose(1, 2)
        if attn == "sdpa":
            a = F.scaled_dot_product_attention(q, k, v, scale=scale)
        else:
            a = ((q * scale) @ k.transpose(-2, -1)).softmax(dim=-1) @ v
        a = lin(a.transpose(1, 2).reshape(B, S, D), "attn.proj")
        x = x + (a if fault == "ls_omitted" else a * w(p + "ls1"))
        m = lin(act(lin(norm(x, "norm2"), "mlp.fc1")), "mlp.fc2")
        x = x + (m if fault == "ls_omitted" else m * w(p + "ls2"))
    return x


def tail(hidden, sd, dtype, ps_version="v2", fault=None, ln_eps=1e-5):
    """extract_feature behind the tower: hidden [B, 1 + g*g, D] -> [B, (g/2)^2, H_llm] in `dtype` (sd: the chat model's `mlp1.*`)"""
    dev = hidden.device
    w = lambda k: sd["mlp1." + k].to(device=dev, dtype=dtype)
    x = hidden.to(dtype)
    g = int((x.shape[1] - 1) ** 0.5)
    assert g * g == x.shape[1] - 1 and g % 2 == 0
    tokens = x[:, :-1, :] if fault == "class_row_kept" else x[:, 1:, :]
    v1 = (ps_version == "v1") != (fault == "v1_for_v2")
    x = shuffle_gather(tokens, g, v1=v1, swap=fault == "chunks_swapped")
    x = F.layer_norm(x, (x.shape[-1],), w("0.weight"), w("0.bias"), ln_eps)
    act = (lambda t: F.gelu(t, approximate="tanh")) if fault == "gelu_tanh" else F.gelu
    return F.linear(act(F.linear(x, w("1.weight"), w("1.bias"))), w("3.weight"), w("3.bias"))


def extract_feature(sd, pixels, cfg, dtype, select_layer=-1, ps_version="v2", attn="naive", fault=None, pos=None):
    """The chat model's extract_feature from its state dict (`vision_model.*`, `mlp1.*`): [B, (g/2)^2, H_llm] in `dtype`"""
    h = tower(sd, pixels, cfg, dtype, select_layer=select_layer, attn=attn, fault=fault, prefix="vision_model.", pos=pos)
    return tail(h, sd, dtype, ps_version=ps_version, fault=fault)


# ---------------------------------------------------------------------------------------------------------------- a stub chat model
def module_tree(sd, dtype=torch.bfloat16, device="cpu"):
    """An nn.Module whose state dict has exactly the names and values of sd: nested plain modules, one parameter per entry"""
    root = torch.nn.Module()
    for k, v in sd.items():
        m, parts = root, k.split(".")
        for part in parts[:-1]:
            if part not in m._modules:
                m.add_module(part, torch.nn.Module())
            m = m._modules[part]
        m.register_parameter(parts[-1], torch.nn.Parameter(v.to(device=device, dtype=dtype), requires_grad=False))
    return root


class StubChatModel(torch.nn.Module):
    """What the hand-off reads of an InternVL2.5 chat model: vision_model (with a config and the reference's parameter names), mlp1,
    select_layer, downsample_ratio, ps_version, and an extract_feature of its own -- the restatement in the parameters' dtype"""

    def __init__(self, sd, cfg=TINY, dtype=torch.bfloat16, device="cpu", select_layer=-1, ps_version="v2"):
        super().__init__()
        self.cfg = dict(cfg)
        self.vision_model = module_tree({k[len("vision_model."):]: v for k, v in sd.items() if k.startswith("vision_model.")}, dtype, device)
        self.vision_model.config = type("InternVisionConfig", (), dict(cfg))()
        self.mlp1 = module_tree({k[len("mlp1."):]: v for k, v in sd.items() if k.startswith("mlp1.")}, dtype, device)
        self.select_layer, self.downsample_ratio, self.ps_version = select_layer, 0.5, ps_version
        self.own_calls = 0
        self.eval()

    def extract_feature(self, pixel_values):
        self.own_calls += 1
        sd = dict(self.state_dict())
        return extract_feature(sd, pixel_values, self.cfg, self.mlp1._modules["0"].weight.dtype, select_layer=self.select_layer,
                               ps_version=self.ps_version)


# ---------------------------------------------------------------------------------------------------------------- the checker
def activation_probe(sd):
    """A second weight set for the checker, from sd: on the test weights the form of the GELU cannot be seen (tanh for erf moves the result
    by 2e-4, far below the bf16 floor of 5e-3), so here every GELU works on its negative tail and its branch carries the result:
      * fc1 and mlp1.1: weights times 1/4, biases -3 -- pre-activations in about [-4, -2], where the tanh form is 0.2 % to 45 % off;
      * fc2 and mlp1.3: no bias; ls2 times 2^15, so that the MLP branch, of size 4e-3, outweighs the residual stream it is added to.
    Every factor is a power of two and -3 is a bf16 value: the weights stay bf16 values."""
    out = dict(sd)
    for k, v in sd.items():
        if k.endswith("mlp.fc1.weight") or k == "mlp1.1.weight":
            out[k] = v * 0.25
        elif k.endswith("mlp.fc1.bias") or k == "mlp1.1.bias":
            out[k] = torch.full_like(v, -3.0)
        elif k.endswith("mlp.fc2.bias") or k == "mlp1.3.bias":
            out[k] = torch.zeros_like(v)
        elif k.endswith(".ls2"):
            out[k] = v * 32768.0
    return out


def check_extract_feature(label, run, sd, pixels, cfg, device="cpu", select_layer=-1, ps_version="v2"):
    """THE checker of the vision path, for the GPU test and for the planted faults alike.  run(weights, pixels) -> [B, T, H_llm] is the
    implementation under test; it is judged on the test weights sd and on activation_probe(sd), each time by the criterion: relative L2
    error against the float64 restatement no worse than 1.5 x that of the bf16 restatement (naive attention, the model's rounding points)
    run with torch on `device`, and below 3e-2.  Prints and returns the measured pairs [(name, e_impl, e_bf16)]; raises AssertionError."""
    pairs = []
    x = pixels.to(device)
    for name, weights in ((label, sd), (label + " [activation probe]", activation_probe(sd))):
        ref = extract_feature(weights, x, cfg, torch.float64, select_layer=select_layer, ps_version=ps_version)
        lib = extract_feature(weights, x, cfg, torch.bfloat16, select_layer=select_layer, ps_version=ps_version)
        got = run(weights, pixels)
        assert got.shape == ref.shape, "%s: shape %s, expected %s" % (name, tuple(got.shape), tuple(ref.shape))
        e_impl, e_lib = rel_l2(got.to(ref.device), ref), rel_l2(lib, ref)
        print("%s: rel-L2 against float64: under test %.3e, bf16 restatement %.3e (ratio %.2f)" % (name, e_impl, e_lib, e_impl / e_lib))
        pairs.append((name, e_impl, e_lib))
    for name, e_impl, e_lib in pairs:
        assert e_impl <= 1.5 * e_lib, "%s: %.3e > 1.5 x bf16 restatement %.3e" % (name, e_impl, e_lib)
        assert e_impl < 3e-2, "%s: %.3e" % (name, e_impl)
    return pairs


# ---------------------------------------------------------------------------------------------------------------- LayerNorm, per element
def shuffle_ln_expect(X, weight, bias, g, eps, v1=False):
    """x2i_internvit_shuffle_ln_bf16 for X bf16 [B, 1 + g*g, D]: (want, bound) float64 [B*(g/2)^2, 4*D].  The bound is tests/ew_ref.py's
    per-element LayerNorm allowance (ln_expect with scale = weight - 1 and shift = bias) plus one f32 rounding of the product with the
    weight, which the affine kernel may keep apart from the final add where the modulated kernel has one fma."""
    from tests import ew_ref as E
    from tests.gemm_ref import U_F32
    x = shuffle_gather(X[:, 1:, :].double(), g, v1=v1).reshape(-1, 4 * X.shape[-1])
    w, b = weight.double().to(x.device), bias.double().to(x.device)
    want, bound, delta = E.ln_expect(x, b, w - 1.0, eps)
    return want, bound + U_F32 * (want - b).abs()
