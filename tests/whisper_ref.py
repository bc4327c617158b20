"""float64 references and helpers for the MiniCPM-o Whisper audio tower's kernels and host module (include/x2i_whisper.h, x2i_amd/whisper.py).
No GPU-only code here: the CPU tests import it too.

  mask      the boolean mask of get_audio_embedding (padding OR NOT chunk), built as the model builds it, and its additive form
  rows      the windows of conv1 and the f32 pooling formula, in torch
  tower     stem, encoder, projector and pooling restated in float64 from a state dict with the checkpoint's key names
  library   the same computation composed from `transformers`' Whisper submodules in the model's order: the library's
            WhisperEncoder.forward ignores attention_mask and insists on all 1500 positions, so its own submodules are called one by one
"""
import torch
import torch.nn as nn

from tests.t5_ref import rel_l2  # noqa: F401  (for the tests that import this module)


def conv_rows(T):
    return (T - 1) // 2 + 1


def token_counts(lens, k):
    """_get_feat_extract_output_lengths: the pooled rows a sample of `len` mel frames keeps"""
    return [((int(n) - 1) // 2 + 1 - k) // k + 1 for n in lens]


# ---------------------------------------------------------------------------------------------------------------- mask
def masked_keys(lens, S, chunk_length):
    """bool [B, S, S], True = key j does NOT count for row i.  The padding part compares post-conv indices with the MEL lengths (the
    model's own oddity); the chunk part lets row i see the keys below (i // C + 1) * C, C = int(chunk_length * 50), when chunk_length > 0."""
    B = len(lens)
    seq = torch.arange(S)[None, :].expand(B, S)
    padding = seq >= torch.tensor([int(n) for n in lens])[:, None].expand(B, S)
    dead = padding[:, None, :].expand(B, S, S)
    if chunk_length > 0:
        C = int(chunk_length * 50)
        chunk = torch.zeros((S, S), dtype=torch.bool)
        for i in range(S):
            chunk[i, 0:min((i // C + 1) * C, S)] = True
        dead = torch.logical_or(dead, torch.logical_not(chunk)[None])
    return dead


def additive_mask(dead, dtype):
    m = torch.zeros(dead.shape, dtype=dtype, device=dead.device)
    m[dead] = float("-inf")
    return m[:, None]


# ---------------------------------------------------------------------------------------------------------------- rows
def mel_rows(mel, Kp=None):
    """[B, Cin, T] -> [B * T, 3 * Cin] in conv1's weight column order (ci, k), with a zero tail up to Kp"""
    B, Cin, T = mel.shape
    rows = torch.nn.functional.pad(mel, (1, 1)).unfold(2, 3, 1).permute(0, 2, 1, 3).reshape(B * T, 3 * Cin)
    if Kp is None:
        return rows
    return torch.cat((rows, torch.zeros((B * T, Kp - 3 * Cin), dtype=mel.dtype, device=mel.device)), 1)


def pool_rows_f32(x, k):
    """bf16 [B, S, D] -> bf16 [B, (S - k) // k + 1, D]: the f32 sum in index order, one division, one rounding"""
    B, S, D = x.shape
    n = (S - k) // k + 1
    v = x[:, :k * n].float().reshape(B, n, k, D)
    acc = v[:, :, 0].clone()
    for i in range(1, k):
        acc = acc + v[:, :, i]
    return (acc / k).bfloat16()


# ---------------------------------------------------------------------------------------------------------------- the whole tower
def gelu_erf_f64(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def tower_reference(sd, mel, lens, *, num_heads, chunk_length, k, eps=1e-5, pool_first=False):
    """float64 restatement of get_audio_embedding from the state dict `sd` (the checkpoint's key names: apm.*, audio_projection_layer.*):
    mel [B, Cin, T], lens the MEL lengths.  -> a list of [n_b, E].  In the model's order: linear2, then the pooling (pool_first: the other
    order, which is the same function)."""
    f = torch.float64
    w = lambda n: sd[n].to(f)
    B, Cin, T = mel.shape
    S, H = conv_rows(T), num_heads
    D = sd["apm.conv1.weight"].shape[0]
    dk = D // H
    x = gelu_erf_f64(mel_rows(mel.to(f)) @ w("apm.conv1.weight").reshape(D, 3 * Cin).t() + w("apm.conv1.bias")).reshape(B, T, D)
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1))
    win = torch.stack([xp[:, kk:kk + 2 * S:2] for kk in range(3)], dim=2).reshape(B * S, 3 * D)               # [.., (k, ci)]
    x = gelu_erf_f64(win @ w("apm.conv2.weight").permute(0, 2, 1).reshape(D, 3 * D).t() + w("apm.conv2.bias")).reshape(B, S, D)
    x = x + w("apm.embed_positions.weight")[:S]
    dead = masked_keys(lens, S, chunk_length)
    ln = lambda t, p: torch.nn.functional.layer_norm(t, (D,), w(p + ".weight"), w(p + ".bias"), eps)
    n = 0
    while "apm.layers.%d.fc1.weight" % n in sd:
        n += 1
    for i in range(n):
        p = "apm.layers.%d." % i
        lin = lambda t, nm: t @ w(p + nm + ".weight").t() + (w(p + nm + ".bias") if p + nm + ".bias" in sd else 0.0)
        h = ln(x, p + "self_attn_layer_norm")
        q, kx, v = (lin(h, "self_attn." + nm).reshape(B, S, H, dk).transpose(1, 2) for nm in ("q_proj", "k_proj", "v_proj"))
        s = (q @ kx.transpose(-1, -2) * dk ** -0.5).masked_fill(dead[:, None], float("-inf"))
        a = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, S, D)
        x = x + lin(a, "self_attn.out_proj")
        h = ln(x, p + "final_layer_norm")
        x = x + lin(gelu_erf_f64(lin(h, "fc1")), "fc2")
    x = ln(x, "apm.layer_norm")
    pl = "audio_projection_layer."
    h = torch.relu(x @ w(pl + "linear1.weight").t() + w(pl + "linear1.bias"))
    pool = lambda t: torch.nn.functional.avg_pool1d(t.transpose(1, 2), k, k).transpose(1, 2)
    lin2 = lambda t: t @ w(pl + "linear2.weight").t() + w(pl + "linear2.bias")
    y = lin2(pool(h)) if pool_first else pool(lin2(h))
    return [y[b, :nb] for b, nb in enumerate(token_counts(lens, k))]


class Projector(nn.Module):
    """The model's MultiModalProjector: three attributes"""

    def __init__(self, in_dim, out_dim):
        super().__init__()
        self.linear1 = nn.Linear(in_dim, out_dim, bias=True)
        self.relu = nn.ReLU()
        self.linear2 = nn.Linear(out_dim, out_dim, bias=True)

    def forward(self, x):
        return self.linear2(self.relu(self.linear1(x)))


def library_tower(D, heads, ffn, layers, n_pos, E, attn="eager", mel_bins=80):
    """(config, `transformers` WhisperEncoder, projector) in float32 on the CPU, their own initialisation under a fixed seed"""
    from transformers.models.whisper.configuration_whisper import WhisperConfig
    from transformers.models.whisper.modeling_whisper import WhisperEncoder
    cfg = WhisperConfig(d_model=D, encoder_attention_heads=heads, encoder_ffn_dim=ffn, encoder_layers=layers, max_source_positions=n_pos,
                        num_mel_bins=mel_bins, activation_function="gelu", decoder_layers=1, decoder_attention_heads=heads, decoder_ffn_dim=8,
                        vocab_size=8, dropout=0.0, attention_dropout=0.0, activation_dropout=0.0)
    cfg._attn_implementation = attn
    torch.manual_seed(0)
    apm = WhisperEncoder(cfg).eval().requires_grad_(False)
    proj = Projector(D, E).eval().requires_grad_(False)
    return cfg, apm, proj


def library_forward(apm, proj, mel, lens, chunk_length, k):
    """get_audio_embedding's computation from the library's own submodules in the model's order: conv1, conv2, embed_positions.weight[:S],
    every WhisperEncoderLayer with the additive mask, layer_norm, the projector, nn.AvgPool1d -> a list of [n_b, E]"""
    w = apm.conv1.weight
    x = mel.to(device=w.device, dtype=w.dtype)
    S = conv_rows(mel.shape[2])
    mask = additive_mask(masked_keys(lens, S, chunk_length).to(w.device), w.dtype)
    with torch.no_grad():
        h = nn.functional.gelu(apm.conv1(x))
        h = nn.functional.gelu(apm.conv2(h))
        h = h.permute(0, 2, 1) + apm.embed_positions.weight[:S]
        for layer in apm.layers:
            h = layer(h, mask)
            h = h[0] if isinstance(h, tuple) else h
        h = apm.layer_norm(h)
        y = nn.AvgPool1d(k, stride=k)(proj(h).transpose(1, 2)).transpose(1, 2)
    return [y[b, :nb] for b, nb in enumerate(token_counts(lens, k))]


def state_dict_of(apm, proj):
    sd = {"apm." + n: v for n, v in apm.state_dict().items()}
    sd.update({"audio_projection_layer." + n: v for n, v in proj.state_dict().items()})
    return sd


def load_state_dict_into(apm, proj, sd):
    apm.load_state_dict({n[4:]: v for n, v in sd.items() if n.startswith("apm.")}, strict=True)
    proj.load_state_dict({n[len("audio_projection_layer."):]: v for n, v in sd.items() if n.startswith("audio_projection_layer.")}, strict=True)


def random_state_dict(apm, proj, seed):
    """The test weights: every matrix and convolution kernel N(0, 1 / fan_in), the position table N(0, 0.02^2); every 1-D tensor -- the norm
    weights and the biases, whose defaults are one and zero and would hide a missing bias -- its default plus 0.1 N(0, 1); float32 tensors
    that hold bf16 values"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for n, v in state_dict_of(apm, proj).items():
        v = v.detach().float().clone()
        if v.dim() == 1:
            v = (torch.ones_like(v) if "norm" in n and n.endswith("weight") else torch.zeros_like(v)) + 0.1 * torch.randn(v.shape, generator=g)
        elif "embed_positions" in n:
            v = 0.02 * torch.randn(v.shape, generator=g)
        else:
            v = torch.randn(v.shape, generator=g) * (v.numel() // v.shape[0]) ** -0.5
        sd[n] = v.bfloat16().float()
    return sd


def random_mel(B, T, lens, seed, mel_bins=80):
    """[B, mel_bins, T] of N(0, 1) holding bf16 values; frames at or beyond a sample's length are zero, as the feature extractor pads"""
    g = torch.Generator().manual_seed(seed)
    mel = torch.randn((B, mel_bins, T), generator=g).bfloat16().float()
    for b, n in enumerate(lens):
        mel[b, :, n:] = 0.0
    return mel


# ---------------------------------------------------------------------------------------------------------------- a stand-in model
class StandInModel(nn.Module):
    """What handoff.HipAudio needs of a MiniCPM-o model: `apm`, `audio_projection_layer`, `audio_avg_pooler`, `audio_encoder_layer`,
    `config.audio_pool_step` and a plain-torch get_audio_embedding(data, chunk_length, dummy) composed from the library's submodules"""

    def __init__(self, apm, proj, k):
        super().__init__()
        self.apm, self.audio_projection_layer, self.audio_avg_pooler = apm, proj, nn.AvgPool1d(k, stride=k)
        self.audio_encoder_layer = -1
        self.config = type("Config", (), dict(audio_pool_step=k, audio_chunk_length=1.0))()
        self.original_calls = 0
        self.eval()

    def get_audio_embedding(self, data, chunk_length=-1, dummy=True):
        self.original_calls += 1
        mel = data.get("audio_features", [])
        raw = data.get("audio_feature_lens", [])
        if len(mel) == 0:
            return [torch.zeros((1, 1))] if self.training and dummy else []
        lens = torch.hstack(raw).tolist()
        flat = library_forward(self.apm, self.audio_projection_layer, mel, lens, chunk_length, self.config.audio_pool_step)
        out, idx = [], 0
        for group in raw:
            out.append(flat[idx:idx + len(group)])
            idx += len(group)
        return out
