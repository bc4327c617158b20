"""ControlNeXtTrainer: the trainable half of the LightControl step on the HIP path (lightcontrol/train_lightcontrol.py:572-588, :672-775).

The reference trains only its 19 `ControlNeXtModel`s (a ModuleList; 6.49 M parameters each) behind a frozen FLUX.1-dev transformer, with
`clip_grad_norm_` over `controlnet.parameters()` and AdamW.  This is the counterpart of `ProjectorTrainer` (x2i_amd/train.py) for that step:
forward with saved activations (`ControlNeXtModel.forward_chained(keep=...)`: the inference code of the chained form itself, handed a dict to
fill -- there is no second statement of the forward), the backward of every net from d loss / d control output, and the optimizer
(`FlatAdamW.step`, x2i_amd/optim.py, shared with `ProjectorTrainer`).  `backward` / `backward_net` take
the gradient in the form `forward_nhwc(add_into=...)` writes the output; x2i_amd/lightcontrol_step.py wires `backward_net` to the injection
points of the transformer's activation-gradient chain (the whole step, loss to AdamW).

Launches of the backward ("ControlNeXt backward"):
  * weight gradients: x2i_conv_wgrad_bf16 for every conv with Cin >= 64 (the 3x3, the 1x1 shortcut and the 2x2 stride-2 projection),
    x2i_conv_stem_wgrad_bf16 for embedding.0, x2i_linear_wgrad_f32 for the time-embedding linears;
  * GroupNorm: x2i_groupnorm_nhwc_bwd_bf16 (dx, d weight, d bias, and d pre_add = the time-embedding term in front of ResnetBlock2D.norm2);
  * data gradients: the forward conv kernel x2i_conv2d_nhwc_bf16 (or the GEMM) on weights repacked here, host-side (the functions below;
    tests/test_controlnext_train_cpu.py checks each against torch.nn.grad.conv2d_input):
      3x3 s1 p1   a 3x3 s1 p1 conv of dY with W'[ci][ky][kx][co] = W[co][ci][2-ky][2-kx]; a residual gradient comes in through `res`;
      3x3 s2 p1   four phase convolutions on the dY grid: input parity 0 sees tap 1 of dY index i, parity 1 taps 2 (of i) and 0 (of i + 1), so the
                  (row, column) phases are 1x1, 1x2, 2x1 and 2x2 convs written interleaved through ldc / out_row_pitch / c_offset;
      1x1         a 1x1 conv of dY with W^T;
      2x2 s2      one GEMM per input-row parity ky: N = 2 Cin covers that row's kx and ci, the rows 2y + ky are written through ldc / batch stride.
    The repacks depend on the weights, which change every step: they are made inside backward() and never cached.
Gradients accumulate in FlatAdamW's ONE flat f32 buffer (one all-reduce per step) until step(); the moments are f32 like ProjectorTrainer's.
"""
import torch

from . import ops
from .ops import ACT_RELU, ACT_SILU
from .optim import EightBitOption, FlatAdamW

# ---------------------------------------------------------------------------------------------------- host-side data-gradient repacks
# (device-agnostic torch index plumbing: they run wherever the weight lives)

# taps of a 3-tap stride-2 pad-1 axis seen by input index 2 i + parity, in the order of dY index i, i + 1
S2_TAPS = ((1,), (2, 0))


def dgrad_weight_3x3(w):
    """Conv2d(Ci -> Co, 3, stride 1, pad 1) weight [Co, Ci, 3, 3] -> packed [Ci, 9 Co] ((ky, kx, co) order) of the 3x3 s1 p1 conv of dY that gives
    dX: W'[ci][ky][kx][co] = W[co][ci][2 - ky][2 - kx]."""
    return w.flip(2, 3).permute(1, 2, 3, 0).reshape(w.shape[1], -1).contiguous()


def dgrad_weights_s2(w):
    """Conv2d(Ci -> Co, 3, stride 2, pad 1) weight [Co, Ci, 3, 3] -> {(py, px): (packed [Ci, KH' KW' Co], KH', KW')}: the stride-1, pad-0 convs on
    the dY grid (zero beyond its last row / column) whose outputs are dX at rows 2 i + py, columns 2 j + px."""
    out = {}
    for py in (0, 1):
        for px in (0, 1):
            ty, tx = list(S2_TAPS[py]), list(S2_TAPS[px])
            sub = w[:, :, ty][:, :, :, tx]
            out[(py, px)] = (sub.permute(1, 2, 3, 0).reshape(w.shape[1], -1).contiguous(), len(ty), len(tx))
    return out


def dgrad_weight_1x1(w):
    """Conv2d(Ci -> Co, 1) weight [Co, Ci, 1, 1] -> [Ci, Co] (the 1x1 conv of dY with W^T)."""
    return w[:, :, 0, 0].t().contiguous()


def dgrad_weights_2x2s2(w):
    """Conv2d(Ci -> Co, 2, stride 2) weight [Co, Ci, 2, 2] -> per input-row parity ky the GEMM weight [2 Ci, Co] whose row kx Ci + ci is
    W[:, ci, ky, kx]: dY [pixels, Co] times its transpose gives the two input pixels (2y + ky, 2x), (2y + ky, 2x + 1) of every dY pixel."""
    return [w[:, :, ky].permute(2, 1, 0).reshape(2 * w.shape[1], w.shape[0]).contiguous() for ky in (0, 1)]


def dgrad_s2(dy, w, oh, ow):
    """dX bf16 [B, 2 oh, 2 ow, Ci] of a 3x3 stride-2 pad-1 conv from dY bf16 [B, oh, ow, Co]: four phase launches of the forward conv kernel."""
    co, ci = w.shape[0], w.shape[1]
    B = dy.shape[0]
    H, W = 2 * oh, 2 * ow
    dx = torch.empty((B, H, W, ci), device=dy.device, dtype=torch.bfloat16)
    for (py, px), (wp, kh, kw) in dgrad_weights_s2(w).items():
        ops.conv2d_nhwc(dy, wp, None, oh, ow, co, ci, kh, kw, 1, 0, out=dx, c_offset=(py * W + px) * ci, c_batch_stride=H * W * ci, ldc=2 * ci,
                        out_row_pitch=2 * W * ci, out_h=oh, out_w=ow)
    return dx


def dgrad_2x2s2(dy, w, B, ho, wo, *, offset=0, ld=None, batch_stride=None):
    """dX bf16 [B, 2 ho, 2 wo, Ci] of a 2x2 stride-2 conv from dY pixel rows [B, ho wo] (row stride ld, batch stride, element offset): per sample
    and input-row parity one GEMM launch with one batch item per dY row."""
    co, ci = w.shape[0], w.shape[1]
    ld = co if ld is None else ld
    bs = ho * wo * ld if batch_stride is None else batch_stride
    H, W = 2 * ho, 2 * wo
    dx = torch.empty((B, H, W, ci), device=dy.device, dtype=torch.bfloat16)
    for ky, wt in enumerate(dgrad_weights_2x2s2(w)):
        for b in range(B):
            ops.gemm(dy, wt, out=dx, M=wo, batch=ho, a_batch_stride=wo * ld, lda=ld, a_offset=offset + b * bs, c_batch_stride=2 * W * ci, ldc=2 * ci,
                     c_offset=b * H * W * ci + ky * W * ci)
    return dx


def _skinny_bwd(dy, W):
    """dx f32 [B, K] = dy f32 [B, N] @ W bf16 [N, K] through x2i_skinny_linear_bwd, in chunks of its 8 rows."""
    if dy.shape[0] <= 8:
        return ops.skinny_linear_bwd(dy.contiguous(), W)
    return torch.cat([ops.skinny_linear_bwd(dy[i:i + 8].contiguous(), W) for i in range(0, dy.shape[0], 8)])


class ControlNeXtTrainer(EightBitOption, FlatAdamW):
    """The control nets of a LightControl step as the trainable side: forward with saves, backward from d loss / d control output, then
    (all-reduce,) global-norm clip over all nets' parameters together (the reference clips controlnet.parameters(), train_lightcontrol.py:769-772)
    and AdamW (:582-588, :773-775).  Parameters stay the nets' bf16 tensors, updated in place; gradients and the two moments are f32 in one flat
    buffer each (FlatAdamW), in the order of the reference ModuleList's named_parameters() ("{i}.<name>"): named_grads() has the key set of
    controlnet.named_parameters() on the ModuleList, which is also what checkpoints.save_control_nets writes.  After the update step() drops
    every net's weight-derived caches (ControlNeXtModel.invalidate_weight_caches) and the saved activations.  `use_8bit_adam=True` (the
    reference's --use_8bit_adam, :559-569) gives the same trainer over FlatAdamW8bit: block-wise 8-bit moments, x2i_amd/optim.py."""

    def __init__(self, nets, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=1.0, process_group=None, *, use_8bit_adam=False):
        self.nets = list(nets)
        super().__init__((("%d.%s" % (i, n), p) for i, net in enumerate(self.nets) for n, p in net.named_parameters()),
                         lr, betas, eps, weight_decay, max_grad_norm, process_group)
        self.saved = None

    def _weights_changed(self):
        for net in self.nets:
            net.invalidate_weight_caches()
        self.saved = None

    @torch.no_grad()
    def forward(self, guided_hint, timestep):
        """Every net's control output (NHWC bf16 [B, H/16, W/16, Cout]; timestep already x 1000, as forward_nhwc takes it), keeping the
        activations the backward needs.  Always the chained form, whatever net.compose says: ControlNeXtModel.forward_chained, i.e. the very
        code ControlNeXtModel.forward runs with compose = False, so bit-identical to it.  Nothing is cached across steps."""
        self.saved = [{} for _ in self.nets]
        return [net.forward_chained(guided_hint, timestep, keep=sv) for net, sv in zip(self.nets, self.saved)]

    @torch.no_grad()
    def backward(self, d_outs, offset=0, batch_stride=None, ld=None):
        """Accumulate every parameter's gradient from d loss / d out of each net: bf16 NHWC / token rows [B, h w, Cout], or any buffer addressed
        like forward_nhwc's add_into (element offset, batch stride, row stride ld)."""
        if self.saved is None:
            raise RuntimeError("ControlNeXtTrainer.backward: call forward first")
        for i, d_out in zip(range(len(self.nets)), d_outs):
            self.backward_net(i, d_out, offset, batch_stride, ld)

    @torch.no_grad()
    def backward_net(self, i, d_out, offset=0, batch_stride=None, ld=None):
        """backward() for net i alone, from d loss / d (its control output) addressed the same way.  The transformer's gradient chain calls this
        at injection i with its residual-stream gradient in place (DistillBackward.backward(on_injection=...): offset = St D, batch stride
        S D, row stride D); d_out is read by the launches enqueued here and may be overwritten by whatever the caller enqueues next."""
        if self.saved is None:
            raise RuntimeError("ControlNeXtTrainer.backward_net: call forward first")
        self._backward_net(i, self.nets[i], self.saved[i], d_out, offset, batch_stride, ld)

    def _backward_net(self, i, net, sv, d_out, offset, batch_stride, ld):
        def g(name):
            return self.g("%d.%s" % (i, name))

        def wgrad(prefix, x, dy, H, W, cin, OH, OW, cout, k, stride, pad, **kw):
            ops.conv_wgrad(x, dy, g(prefix + ".weight"), g(prefix + ".bias"), H, W, cin, OH, OW, cout, k, k, stride, pad, accumulate=True, **kw)

        def gn(prefix, x, dy, G, eps, **kw):
            mod = _resolve(net, prefix)
            return ops.groupnorm_bwd(x, dy, mod.weight, mod.bias, G, eps, dw=g(prefix + ".weight"), db=g(prefix + ".bias"), accumulate=True, **kw)

        def dgrad3(dy, conv, H, W, res=None):
            co, ci = conv.weight.shape[0], conv.weight.shape[1]
            return ops.conv2d_nhwc(dy, dgrad_weight_3x3(conv.weight), None, H, W, co, ci, 3, 3, 1, 1, res=res)

        B, h, w = sv["B"], sv["h"], sv["w"]
        h2, w2, h3, w3 = h // 2, w // 2, h // 4, w // 4
        ho, wo = h3 // 2, w3 // 2
        g0, g1 = net.groups
        f32 = dict(device=d_out.device, dtype=torch.float32)
        fin = net.mid_convs[1]
        co = fin.weight.shape[0]
        ld = co if ld is None else ld
        bs = ho * wo * ld if batch_stride is None else batch_stride
        # mid_convs.1 (2 x 2, stride 2)
        wgrad("mid_convs.1", sv["xm"], d_out, h3, w3, 256, ho, wo, co, 2, 2, 0, dy_offset=offset, dy_batch_stride=bs, ldy=ld, B=B)
        dxm = dgrad_2x2s2(d_out, fin.weight, B, ho, wo, offset=offset, ld=ld, batch_stride=bs)
        # mid_convs.0 + the residual: xm = GN4(conv3(GN2(relu(conv0(xd1))))) + xd1
        m = net.mid_convs[0]
        dy3 = gn("mid_convs.0.4", sv["y3"], dxm, 8, 1e-5)
        wgrad("mid_convs.0.3", sv["y2"], dy3, h3, w3, 256, h3, w3, 256, 3, 1, 1)
        dy2 = dgrad3(dy3, m[3], h3, w3)
        dp0 = gn("mid_convs.0.2", sv["y0"], dy2, 8, 1e-5, in_relu=True)
        wgrad("mid_convs.0.0", sv["xd1"], dp0, h3, w3, 256, h3, w3, 256, 3, 1, 1)
        dxd1 = dgrad3(dp0, m[0], h3, w3, res=dxm)
        # down_sample.1 (3 x 3, stride 2)
        wgrad("down_sample.1.conv", sv["xr1"], dxd1, h2, w2, 256, h3, w3, 256, 3, 2, 1)
        dxr1 = dgrad_s2(dxd1, net.down_sample[1].conv.weight, h3, w3)
        # down_res.1: xr1 = conv2(silu(GN(conv1(silu(GN(xd0))) + tproj1))) + conv_shortcut(xd0)
        r = net.down_res[1]
        wgrad("down_res.1.conv2", sv["n2b"], dxr1, h2, w2, 256, h2, w2, 256, 3, 1, 1)
        dn2b = dgrad3(dxr1, r.conv2, h2, w2)
        wgrad("down_res.1.conv_shortcut", sv["xd0"], dxr1, h2, w2, 128, h2, w2, 256, 1, 1, 0)
        dxd0 = ops.conv2d_nhwc(dxr1, dgrad_weight_1x1(r.conv_shortcut.weight), None, h2, w2, 256, 128, 1, 1, 1, 0)
        dtp1 = torch.empty((B, r.time_emb_proj.weight.shape[0]), **f32)
        dh1b = gn("down_res.1.norm2", sv["h1b"], dn2b, g1, 1e-6, act=ACT_SILU, pre_add=sv["tp1"], dpre=dtp1)
        wgrad("down_res.1.conv1", sv["n1b"], dh1b, h2, w2, 128, h2, w2, 256, 3, 1, 1)
        dn1b = dgrad3(dh1b, r.conv1, h2, w2)
        dxd0 = gn("down_res.1.norm1", sv["xd0"], dn1b, g1, 1e-6, act=ACT_SILU, dx_in=dxd0, dx=dxd0)
        # down_sample.0
        wgrad("down_sample.0.conv", sv["xr0"], dxd0, h, w, 128, h2, w2, 128, 3, 2, 1)
        dxr0 = dgrad_s2(dxd0, net.down_sample[0].conv.weight, h2, w2)
        # down_res.0 (identity shortcut): xr0 = conv2(silu(GN(conv1(silu(GN(x0))) + tproj0))) + x0
        r = net.down_res[0]
        wgrad("down_res.0.conv2", sv["n2"], dxr0, h, w, 128, h, w, 128, 3, 1, 1)
        dn2 = dgrad3(dxr0, r.conv2, h, w)
        dtp0 = torch.empty((B, r.time_emb_proj.weight.shape[0]), **f32)
        dh1 = gn("down_res.0.norm2", sv["h1"], dn2, g0, 1e-6, act=ACT_SILU, pre_add=sv["tp0"], dpre=dtp0)
        wgrad("down_res.0.conv1", sv["n1"], dh1, h, w, 128, h, w, 128, 3, 1, 1)
        dn1 = dgrad3(dh1, r.conv1, h, w)
        dx0 = gn("down_res.0.norm1", sv["x0"], dn1, g0, 1e-6, act=ACT_SILU, dx_in=dxr0)
        # embedding: conv s2 (stem), GN, ReLU, conv, GN, ReLU, conv, GN, ReLU
        e = net.embedding
        ds6 = gn("embedding.7", sv["s6"], dx0, 2, 1e-5, act=ACT_RELU)
        wgrad("embedding.6", sv["a3"], ds6, h, w, 64, h, w, 128, 3, 1, 1)
        da3 = dgrad3(ds6, e[6], h, w)
        ds3 = gn("embedding.4", sv["s3"], da3, 2, 1e-5, act=ACT_RELU)
        wgrad("embedding.3", sv["a0"], ds3, h, w, 64, h, w, 64, 3, 1, 1)
        da0 = dgrad3(ds3, e[3], h, w)
        ds0 = gn("embedding.1", sv["s0"], da0, 2, 1e-5, act=ACT_RELU)
        ops.conv_stem_wgrad(sv["img"], ds0, g("embedding.0.weight"), g("embedding.0.bias"), accumulate=True)
        # time embedding: tproj_k = time_emb_proj_k(silu(emb)), emb = linear_2(silu(linear_1(tp)))
        r0, r1, te = net.down_res[0], net.down_res[1], net.time_embedding
        ops.linear_wgrad(dtp0, sv["emb"], g("down_res.0.time_emb_proj.weight"), g("down_res.0.time_emb_proj.bias"), act_in=ACT_SILU, accumulate=True)
        ops.linear_wgrad(dtp1, sv["emb"], g("down_res.1.time_emb_proj.weight"), g("down_res.1.time_emb_proj.bias"), act_in=ACT_SILU, accumulate=True)
        demb = _skinny_bwd(torch.cat([dtp0, dtp1], 1), torch.cat([r0.time_emb_proj.weight, r1.time_emb_proj.weight], 0))
        ops.act_bwd_(demb, sv["emb"], ACT_SILU)
        ops.linear_wgrad(demb, sv["e1"], g("time_embedding.linear_2.weight"), g("time_embedding.linear_2.bias"), accumulate=True)
        de1 = _skinny_bwd(demb, te.linear_2.weight)
        ops.act_bwd_(de1, sv["pre1"], ACT_SILU)
        ops.linear_wgrad(de1, sv["tp"], g("time_embedding.linear_1.weight"), g("time_embedding.linear_1.bias"), accumulate=True)


def _resolve(net, dotted):
    mod = net
    for part in dotted.split("."):
        mod = mod[int(part)] if part.isdigit() else getattr(mod, part)
    return mod
