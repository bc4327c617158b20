"""The MiniCPM-o Whisper audio tower on the HIP path: `model.apm` (MiniCPMWhisperEncoder, Whisper's encoder), `audio_projection_layer`
(linear, ReLU, linear to the LLM width) and `audio_avg_pooler` (AvgPool1d(k, stride=k)) of MiniCPM-o 2.6 -- what get_audio_embedding runs
whenever a prompt holds audio (audio2image).

A call holds B mel spectrograms [B, 80, T], sample b with len_b <= T valid mel frames.  The stem halves the time axis:
S = (T - 1) // 2 + 1 tokens.  Key j of sample b counts for query row i iff j < len_b and j < (i // C + 1) * C with C the chunk's frames
(C <= 0: no chunking) -- the reference compares the MEL length len_b with POST-CONV indices, and so does this module: the key range of row
i is [0, min(len_b, S, (i // C + 1) * C)), a key range per row, which is all x2i_vit_attention_bf16 knows of it.  Sample b keeps the first
n_b = (S_b - k) // k + 1 pooled rows, S_b = (len_b - 1) // 2 + 1.

Launch list (every launch in libx2i_hip.so; include/x2i_whisper.h, x2i_siglip.h, x2i_vit.h and x2i.h):
  mel_rows       the windows of conv1 as rows [B*T, Kp = 256]                                          x2i_whisper_mel_rows_bf16
  gemm           conv1 + bias + GELU(erf), written one row into a buffer of T + 2 rows per sample      x2i_gemm_bf16
  gemm           conv2 (stride 2) + bias + GELU(erf): A = that buffer read as OVERLAPPING rows, lda = 2*D, K = 3*D; no kernel, no copy
  add_positions  + embed_positions[:S], in place                                                       x2i_siglip_add_positions_bf16
  per layer, eight launches:
  ln_affine      self_attn_layer_norm                                                                  x2i_ln_affine_bf16
  gemm           q | k | v + bias (the k slice of the packed bias is zero: k_proj has none)
  head_split     -> Q, K [B,H,Spad,64], V^T [B,H,64,Spad]                                              x2i_siglip_head_split_bf16
  attention      keys [0, row_hi), scale = 64 ** -0.5                                                  x2i_vit_attention_bf16
  gemm           out_proj + bias + residual (one rounding)
  ln_affine      final_layer_norm
  gemm           fc1 + bias + GELU(erf)
  gemm           fc2 + bias + residual
  ln_affine      layer_norm
  gemm           linear1 + bias + ReLU
  pool_rows      AvgPool1d(k, k) over time                                                             x2i_whisper_pool_rows_bf16
  gemm           linear2 + bias, on the pooled rows

The pooling stands BEFORE linear2: averaging is linear and leaves the bias alone, so this is the reference's linear2-then-pool with
linear2's work divided by k.  The position table is added by its own launch, after conv2's GELU was rounded -- the reference's two
roundings: the GEMM instantiates no epilogue with an activation AND a residual, and this module does not add one.

Packed storage.  The parameters carry the checkpoint's names (`apm.*`, `audio_projection_layer.*`), so those slices of a MiniCPM-o state
dict load strictly:
  * conv1.weight [D, 80, 3] is the first 240 columns of a [D, Kp = 256] matrix whose other columns are zero (a view): the GEMM's fast
    path needs K % 64 == 0.
  * q_proj / k_proj / v_proj are views of one [3*D, D] weight, and q_proj.bias / v_proj.bias of one [3*D] bias whose k slice is zero.
  * conv2.weight [D, D, 3] has a COPY permuted to [D, 3*D] in (k, ci) order, the column order of the overlapping rows; made at load and
    again in _apply; pack_() makes it again after the parameter was written in place.
"""
import torch
import torch.nn as nn

from . import ops, siglip_ops, vit_ops, whisper_ops
from ._packed import WB, PackedModule, config_fields, config_object

_FIELDS = dict(d_model=1024, encoder_attention_heads=16, encoder_ffn_dim=4096, encoder_layers=24, max_source_positions=1500, num_mel_bins=80,
               activation_function="gelu", embed_dim=3584, pool_step=2, layer_norm_eps=1e-5)


def conv_rows(T):
    """Tokens the stem makes of T mel frames: Conv1d(3, stride=2, padding=1) after Conv1d(3, padding=1)"""
    return (T - 1) // 2 + 1


def token_counts(feature_lens, k):
    """[n_b]: the pooled rows sample b keeps, the reference's _get_feat_extract_output_lengths"""
    return [whisper_ops.pooled_rows(conv_rows(int(n)), k) for n in feature_lens]


def key_ranges(feature_lens, S, chunk_frames):
    """int32 [B, S]: row_hi, the end of the key range [0, row_hi) of every query row -- min(len_b, S, (i // C + 1) * C); C <= 0: no chunks.
    len_b is the MEL length and S counts post-conv rows, as in the reference."""
    lens = torch.tensor([int(n) for n in feature_lens], dtype=torch.int64)[:, None].clamp(max=S)
    hi = lens.expand(len(feature_lens), S)
    if chunk_frames > 0:
        hi = torch.minimum(hi, ((torch.arange(S) // chunk_frames + 1) * chunk_frames)[None, :])
    return hi.to(torch.int32).contiguous()


class WhisperPlan:
    """Everything of a call that depends on (feature_lens, T, chunk_frames) alone (WhisperAudioTower.plan)"""


class WhisperAudioTower(PackedModule):
    """Drop-in for get_audio_embedding's tensor work.  forward(mel [B, 80, T], feature_lens) -> (bf16 [B, n_max, E], [n_b]): sample b's
    audio embedding is rows < n_b of out[b].  Eval only."""

    _eval_only = True
    _copies = "_conv2"

    def __init__(self, config=None, device="cuda", dtype=torch.bfloat16, **kw):
        super().__init__(device)
        f = config_fields(_FIELDS, config, kw, "WhisperAudioTower")
        if dtype != torch.bfloat16:
            raise ValueError("x2i_amd: the HIP path computes in bf16 (fp32 statistics/accumulation)")
        if f["activation_function"] != "gelu":
            raise ValueError("x2i_amd WhisperAudioTower: activation_function=%r is not built (gelu, the erf form, only)" % (f["activation_function"],))
        D, H, F, NL, E = f["d_model"], f["encoder_attention_heads"], f["encoder_ffn_dim"], f["encoder_layers"], f["embed_dim"]
        Cin, NP, k = f["num_mel_bins"], f["max_source_positions"], f["pool_step"]
        if H <= 0 or D != 64 * H:
            raise ValueError("x2i_amd WhisperAudioTower: the tower's heads are 64 wide (got d_model=%r, encoder_attention_heads=%r)" % (D, H))
        if F <= 0 or F % 8 or NL < 1 or E <= 0 or E % 8 or Cin < 1 or NP < 1:
            raise ValueError("x2i_amd WhisperAudioTower: need a layer, encoder_ffn_dim and embed_dim positive multiples of 8, a mel bin and a position")
        if not 1 <= k <= 8:
            raise ValueError("x2i_amd WhisperAudioTower: pool_step must be in 1..8 (got %r)" % (k,))
        f["head_dim"] = 64
        self.config = config_object("WhisperAudioTowerConfig", f)
        self.Kp = Kp = siglip_ops.pad64(3 * Cin)
        self._conv2 = None
        param, view = self._param, self._view
        self._store("c1", D, Kp, zero=True)
        apm = nn.Module()
        apm.add_module("conv1", WB(view("c1", (slice(None), slice(0, 3 * Cin)), (D, Cin, 3)), param(D)))
        apm.add_module("conv2", WB(param(D, D, 3), param(D)))
        apm.add_module("embed_positions", WB(param(NP, D)))
        layers = []
        for i in range(NL):
            self._store("%d.qkv.w" % i, 3 * D, D, zero=True)
            self._store("%d.qkv.b" % i, 3 * D, zero=True)
            att = nn.Module()
            for j, nm in enumerate(("q_proj", "k_proj", "v_proj")):
                rows = slice(j * D, (j + 1) * D)
                att.add_module(nm, WB(view("%d.qkv.w" % i, rows), None if nm == "k_proj" else view("%d.qkv.b" % i, rows)))
            att.add_module("out_proj", WB(param(D, D), param(D)))
            layer = nn.Module()
            layer.add_module("self_attn", att)
            layer.add_module("self_attn_layer_norm", WB(param(D), param(D)))
            layer.add_module("fc1", WB(param(F, D), param(F)))
            layer.add_module("fc2", WB(param(D, F), param(D)))
            layer.add_module("final_layer_norm", WB(param(D), param(D)))
            layers.append(layer)
        apm.add_module("layers", nn.ModuleList(layers))
        apm.add_module("layer_norm", WB(param(D), param(D)))
        self.apm = apm
        self.audio_projection_layer = nn.Module()
        self.audio_projection_layer.add_module("linear1", WB(param(E, D), param(E)))
        self.audio_projection_layer.add_module("linear2", WB(param(E, E), param(E)))
        self.eval()

    @torch.no_grad()
    def pack_(self):
        """conv2's weight [D, D, 3] as the [D, 3*D] matrix in (k, ci) column order that the overlapping rows meet (the module docstring), from
        the parameter as it is now"""
        w = self.apm.conv2.weight
        self._conv2 = w.permute(0, 2, 1).reshape(w.shape[0], 3 * w.shape[1]).contiguous()
        return self

    @classmethod
    def from_hf(cls, apm, projector, pool_step, device=None):
        """A bf16 copy of instantiated modules -- the model's `apm` (or a `transformers` WhisperEncoder) and its `audio_projection_layer` --
        on `device` (default: the tower's); pool_step: the model's config.audio_pool_step"""
        w = apm.layer_norm.weight
        device = w.device if device is None else torch.device(device)
        m = cls(apm.config, device=device, embed_dim=projector.linear1.out_features, pool_step=int(pool_step))
        sd = {"apm." + k: v for k, v in apm.state_dict().items()}
        sd.update({"audio_projection_layer." + k: v for k, v in projector.state_dict().items()})
        m.load_state_dict({k: v.detach().to(device=device, dtype=torch.bfloat16) for k, v in sd.items()}, strict=True)
        return m

    def init_random_(self, seed=0):
        """Random weights in place (tools; there are no checkpoints offline): matrices and convolutions N(0, 1 / fan_in), the position
        table N(0, 0.02^2), biases 0.1 N(0, 1), norm weights 1 + 0.1 N(0, 1)"""
        def rule(n, p, r):
            if n.endswith("embed_positions.weight"):
                return 0.02 * r
            if "norm" in n and n.endswith(".weight"):
                return 1.0 + 0.1 * r
            return 0.1 * r if p.dim() == 1 else r * (p.numel() // p.shape[0]) ** -0.5

        self._init_random(seed, rule)
        return self.pack_()

    # ------------------------------------------------------------------ plan
    @torch.no_grad()
    def plan(self, feature_lens, T, chunk_frames=50):
        """All the host work of a call, once per (lengths, T, chunk): S, the key ranges, the token counts and the workspaces, with the two pad
        rows of conv1's output zeroed.  feature_lens: the B mel lengths (a list, or a tensor: ONE host read), each in 1..T; T: mel frames of
        the batch; chunk_frames: C (<= 0: no chunking).  The result lives on the module's device and is valid until the module moves."""
        c = self.config
        lens = tuple(int(v) for v in (feature_lens.reshape(-1).tolist() if isinstance(feature_lens, torch.Tensor) else feature_lens))
        T, C = int(T), int(chunk_frames)
        if T < 1:
            raise ValueError("x2i_amd WhisperAudioTower: T = %d mel frames; at least one is needed" % T)
        if not lens or any(n < 1 or n > T for n in lens):
            raise ValueError("x2i_amd WhisperAudioTower: feature_lens must be mel lengths in 1..T = %d (got %r)" % (T, lens))
        S = conv_rows(T)
        if S > c.max_source_positions:
            raise ValueError("x2i_amd WhisperAudioTower: T = %d mel frames are S = %d tokens, beyond the %d rows of embed_positions"
                             % (T, S, c.max_source_positions))
        dev = self.device
        B, D, H, F, E, k = len(lens), c.d_model, c.encoder_attention_heads, c.encoder_ffn_dim, c.embed_dim, c.pool_step
        p = WhisperPlan()
        p.lens, p.T, p.S, p.B, p.chunk_frames, p.device = lens, T, S, B, C, dev
        p.Spad = Spad = whisper_ops.pad64(S)
        p.counts = token_counts(lens, k)
        p.n_max = whisper_ops.pooled_rows(S, k)
        hi = key_ranges(lens, S, C)
        p.key_hi = hi                                          # (on the CPU, for the tests)
        p.row_lo = torch.zeros((B, S), dtype=torch.int32, device=dev)
        p.row_hi = hi.to(dev)
        p.ids = torch.arange(S, dtype=torch.int32).repeat(B).to(dev)
        if dev.type == "cuda":
            bf = dict(device=dev, dtype=torch.bfloat16)
            M = B * S
            # C1 is zeroed once: conv1's GEMM writes rows 1 .. T of each sample, and rows 0 and T + 1 are the padding conv2's rows read.
            # Q, K, V^T are zeroed once: head_split writes rows / columns s < S only, and the attention kernel needs K and V^T finite up to Spad
            p.ws = dict(XR=torch.empty((B * T, self.Kp), **bf), C1=torch.zeros((B, T + 2, D), **bf), X=torch.empty((M, D), **bf),
                        NRM=torch.empty((M, D), **bf), QKV=torch.empty((M, 3 * D), **bf), Q=torch.zeros((B, H, Spad, 64), **bf),
                        K=torch.zeros((B, H, Spad, 64), **bf), VT=torch.zeros((B, H, 64, Spad), **bf), ATT=torch.empty((M, D), **bf),
                        HH=torch.empty((M, F), **bf), P1=torch.empty((M, E), **bf), PL=torch.empty((B * max(p.n_max, 1), E), **bf))
        return p

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward(self, mel, feature_lens=None, chunk_frames=50, plan=None):
        """mel: [B, num_mel_bins, T] (any float dtype; rounded to bf16), on the module's device.  feature_lens: the B mel lengths (default:
        all T).  -> (bf16 [B, n_max, E], [n_b]): rows >= n_b of a sample are finite and mean nothing.  With a plan
        (self.plan(feature_lens, T, chunk_frames)) the call only enqueues: no host read, no synchronisation, one allocation (the result).
        Without one, the lengths are read once and the plan of the last shape is kept."""
        c = self.config
        D, H, E, k, eps = c.d_model, c.encoder_attention_heads, c.embed_dim, c.pool_step, c.layer_norm_eps
        if mel.dim() != 3 or mel.shape[1] != c.num_mel_bins or not mel.shape[0]:
            raise ValueError("x2i_amd WhisperAudioTower: mel must be [B, %d, T] (got %s)" % (c.num_mel_bins, tuple(mel.shape)))
        B, _, T = mel.shape
        if T < 1:
            raise ValueError("x2i_amd WhisperAudioTower: T = %d mel frames; at least one is needed" % T)
        if plan is None:
            if feature_lens is None:
                lens = (T,) * B
            else:
                lens = tuple(int(v) for v in (feature_lens.reshape(-1).tolist() if isinstance(feature_lens, torch.Tensor) else feature_lens))   # the one host read
            if len(lens) != B:
                raise ValueError("x2i_amd WhisperAudioTower: %d feature_lens for %d spectrograms" % (len(lens), B))
            plan = self._plan_for(lens, T, int(chunk_frames))
        if (plan.B, plan.T) != (B, T):
            raise ValueError("x2i_amd WhisperAudioTower: the plan is for %d spectrograms of %d frames, mel holds %d of %d" % (plan.B, plan.T, B, T))
        if plan.device != self.device or not hasattr(plan, "ws"):
            raise ValueError("x2i_amd WhisperAudioTower: the plan was made on %s; the module is on %s and runs on the GPU only" % (plan.device, self.device))
        if mel.device != self.device:
            raise ops._lib.X2IError("x2i_amd: mel must live on the model's device (got %s)" % mel.device)
        if self._conv2 is None:
            self.pack_()
        if mel.dtype != torch.bfloat16:
            mel = mel.to(torch.bfloat16)
        if T > 1 and mel.stride(2) != 1:
            mel = mel.contiguous()
        ws, apm, proj = plan.ws, self.apm, self.audio_projection_layer
        XR, C1, X, NRM, QKV, Q, K, VT, ATT, HH, P1, PL = (ws[n] for n in ("XR", "C1", "X", "NRM", "QKV", "Q", "K", "VT", "ATT", "HH", "P1", "PL"))
        S, Spad, Kp, M = plan.S, plan.Spad, self.Kp, B * plan.S
        whisper_ops.mel_rows(mel, XR, Kp)
        ops.gemm(XR, self._fused["c1"], apm.conv1.bias, out=C1, M=T, batch=B, a_batch_stride=T * Kp, c_offset=D, c_batch_stride=(T + 2) * D,
                 act=ops.ACT_GELU_ERF)
        ops.gemm(C1, self._conv2, apm.conv2.bias, out=X, M=S, batch=B, lda=2 * D, a_batch_stride=(T + 2) * D, c_batch_stride=S * D,
                 act=ops.ACT_GELU_ERF)
        siglip_ops.add_positions(X, plan.ids, apm.embed_positions.weight)
        for i, layer in enumerate(apm.layers):
            ops.ln_affine(X, layer.self_attn_layer_norm.weight, layer.self_attn_layer_norm.bias, eps, out=NRM)
            ops.gemm(NRM, self._fused["%d.qkv.w" % i], self._fused["%d.qkv.b" % i], out=QKV, M=M)
            siglip_ops.head_split(QKV, Q, K, VT, B, S, Spad, H, 64)
            vit_ops.attention(Q, K, VT, ATT, B, H, S, Spad, 64, 0.125, D, S * D, plan.row_lo, plan.row_hi)
            ops.gemm(ATT, layer.self_attn.out_proj.weight, layer.self_attn.out_proj.bias, out=X, res=X, M=M)
            ops.ln_affine(X, layer.final_layer_norm.weight, layer.final_layer_norm.bias, eps, out=NRM)
            ops.gemm(NRM, layer.fc1.weight, layer.fc1.bias, out=HH, M=M, act=ops.ACT_GELU_ERF)
            ops.gemm(HH, layer.fc2.weight, layer.fc2.bias, out=X, res=X, M=M)
        ops.ln_affine(X, apm.layer_norm.weight, apm.layer_norm.bias, eps, out=NRM)
        n = plan.n_max
        out = torch.empty((B, n, E), device=self.device, dtype=torch.bfloat16)
        if n:
            ops.gemm(NRM, proj.linear1.weight, proj.linear1.bias, out=P1, M=M, act=ops.ACT_RELU)
            whisper_ops.pool_rows(P1, PL, B, S, E, k)
            ops.gemm(PL, proj.linear2.weight, proj.linear2.bias, out=out, M=B * n)
        return out, list(plan.counts)
