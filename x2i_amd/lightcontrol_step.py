"""One LightControl training step on the HIP path, from packed latents to updated control-net weights
(lightcontrol/train_lightcontrol.py:672-775).

The reference trains its 19 ControlNeXt nets behind a frozen FLUX.1-dev transformer with a flow-matching loss.  The parts:

  sample_timesteps / sigmas_for   the logit-normal timestep density (:693-701) and get_sigmas (:412-420) on the scheduler's training tables
  x2i_flow_match_noise_bf16       noisy = (1 - sigma) x + sigma noise and target = noise - x with the reference's bf16 roundings, written as
                                  packed tokens (:706-714, :756); `flow_match_noise_reference` below is its torch restatement
  ControlNeXtTrainer.forward      every net's control output with the activations its backward needs (ControlNeXtModel.forward_chained
                                  with a dict to keep them in; x2i_amd/lightcontrol_train.py)
  DistillBackward.forward_train   the transformer forward with saves; net i's output is added into the image rows behind double block i
  x2i_mse_loss_grad_bf16          loss = mean((noise_pred - target)^2) (:758-762, weighting "none") and d noise_pred.  The mean over samples
                                  of per-sample means is the overall mean (equal sizes), and unpacking is a permutation, so the loss on
                                  packed rows is the reference's loss on unpacked latents
  DistillBackward.backward        seeded at d noise_pred: proj_out, norm_out, the single blocks and the double blocks down to injection 0; at
                                  every injection the image rows of the residual-stream gradient ARE d loss / d control output i
                                  (hidden += out * 1.0) and go to ControlNeXtTrainer.backward_net in place -- no snapshots; the chain stops
                                  behind injection 0 (what lies below is frozen, and no control output depends on it)
  ControlNeXtTrainer.step         global-norm clip over all nets, AdamW (:769-775): FlatAdamW.step (x2i_amd/optim.py), or with
                                  ControlNeXtTrainer(use_8bit_adam=True) FlatAdamW8bit.step, the block-wise 8-bit moments that stand where
                                  the reference's --use_8bit_adam selects bnb.optim.AdamW8bit (:559-569)

The transformer stays frozen: no weight gradient of it is computed.  VAE encoding of the target image is the caller's business
(x2i_amd.vae.AutoencoderKL(with_encoder=True)); the training program around the step (arguments, data, lr schedule, checkpoint loop) and the MLLM
that makes the prompt embeddings are out of scope; checkpoints.save_control_nets writes the nets.
"""
import torch

from . import ops
from .pipeline import FluxPipeline
from .train import DistillBackward


def flow_match_noise_reference(latents, noise, sigmas):
    """The semantics of ops.flow_match_noise as the torch expression of train_lightcontrol.py:705-714, :756 (any device, any dtype; on bf16
    tensors every operation rounds, which is what the kernel reproduces bit for bit): latents, noise [B, C, h, w], sigmas [B] ->
    (packed noisy model input, packed target), both [B, (h/2)(w/2), 4C]."""
    B, Cc, h, w = latents.shape
    s = sigmas.to(device=latents.device, dtype=latents.dtype).reshape(B, 1, 1, 1)
    noisy = (1.0 - s) * latents + s * noise
    target = noise - latents
    return FluxPipeline._pack_latents(noisy, B, Cc, h, w), FluxPipeline._pack_latents(target, B, Cc, h, w)


def sample_timesteps(scheduler, batch_size, generator=None):
    """One training timestep per image from the logit-normal density with mean 0, std 1 (compute_density_for_timestep_sampling, :693-701):
    u = sigmoid(randn), indices = (u * num_train_timesteps).long(), timesteps = scheduler.timesteps[indices].  `scheduler` holds its TRAINING
    tables (a FlowMatchEulerDiscreteScheduler on which set_timesteps has not been called, the reference's noise_scheduler_copy)."""
    n = scheduler.config.num_train_timesteps
    if scheduler.timesteps.numel() != n:
        raise ValueError("sample_timesteps: the scheduler holds an inference schedule; pass one with its training tables")
    u = torch.sigmoid(torch.randn((batch_size,), generator=generator, device=generator.device if generator is not None else "cpu"))
    indices = (u * n).long().clamp_(max=n - 1).to(scheduler.timesteps.device)
    return scheduler.timesteps[indices]


def sigmas_for(scheduler, timesteps):
    """get_sigmas (:412-420): the sigma of every timestep by table lookup, f32 [B]."""
    table = scheduler.timesteps
    idx = [int((table == t).nonzero().item()) for t in timesteps.to(table.device)]
    return scheduler.sigmas[idx].flatten().to(torch.float32)


def add_control_outputs(outs):
    """The control callable of DistillBackward.forward_train / FluxTransformer2DModel.denoise for control outputs that exist already:
    (i, timestep_x1000, X, St, S, D) adds outs[i] (bf16 [B, ..., D], Si rows per sample) into the image rows of X [B, S, D]; False when
    there is no output i."""
    def control(i, t1000, X, St, S, D):
        if i >= len(outs):
            return False
        B, Si = X.shape[0], S - St
        o = outs[i]
        if o.dtype != torch.bfloat16 or o.numel() != B * Si * D or o.shape[-1] != D or not o.is_contiguous():
            raise ValueError("control output %d: expected contiguous bf16 [%d, %d rows, %d], got %s" % (i, B, Si, D, tuple(o.shape)))
        ops.gate_bwd(X, None, None, o, X, None, B=B, S=Si, D=D, R=8, dx_bs=S * D, g_bs=Si * D, dt_bs=S * D, dx_offset=St * D, dt_offset=St * D)
        return True
    return control


class LightControlTrainStep:
    """The step of the module docstring for a frozen x2i_amd FluxTransformer2DModel and a ControlNeXtTrainer over its control nets."""

    def __init__(self, transformer, trainer):
        if len(trainer.nets) > transformer.config.num_layers:
            raise ValueError("LightControlTrainStep: more control nets than double-stream blocks")
        self.transformer, self.trainer = transformer, trainer
        self.chain = DistillBackward(transformer)
        self.mark = None   # optional callable(name), called where a phase of the step has been enqueued (tools/lightcontrol_train_bench.py)

    def _mark(self, name):
        if self.mark is not None:
            self.mark(name)

    def _on_injection(self, i, dX, St, S, D):
        self._mark("transformer backward")
        self.trainer.backward_net(i, dX, offset=St * D, batch_stride=S * D, ld=D)
        self._mark("control backward")

    @torch.no_grad()
    def __call__(self, latents, noise, timesteps, sigmas, prompt_embeds, pooled_prompt_embeds, guided_hint, guidance_scale=3.5,
                 optimizer_step=True, grad_scale=1.0):
        """latents: the VAE-encoded, shifted and scaled image [B, 16, h, w]; noise like it; timesteps [B] as sample_timesteps gives them
        (0..1000), sigmas [B] (sigmas_for); prompt_embeds [B, St, joint_dim], pooled_prompt_embeds [B, pooled_dim]; guided_hint [B, 3, H, W]
        with H / 16 = h / 2.  Gradients accumulate in the trainer (scaled by grad_scale) until a call with optimizer_step=True.  Returns the
        loss, a device f32 scalar."""
        m, tr = self.transformer, self.trainer
        dev = m.device
        bf = dict(device=dev, dtype=torch.bfloat16)
        B, Cc, h, w = latents.shape
        # 1. conditioning: txt_ids zeros (:727), img_ids of the packed grid (:689), guidance expanded to the batch (:728-729)
        txt_ids = torch.zeros((prompt_embeds.shape[1], 3), device=dev, dtype=torch.float32)
        img_ids = FluxPipeline._prepare_latent_image_ids(B, h // 2, w // 2, dev, torch.float32)
        guidance = torch.full((B,), float(guidance_scale), device=dev, dtype=torch.float32) if m.config.guidance_embeds else None
        st = self.chain.prepare_conditioning(prompt_embeds.to(**bf), pooled_prompt_embeds.to(**bf), txt_ids, img_ids, guidance)
        # 2. noisy model input and target, packed
        noisy, target = ops.flow_match_noise(latents.to(**bf).contiguous(), noise.to(**bf).contiguous(),
                                             sigmas.to(device=dev, dtype=torch.float32).reshape(B).contiguous())
        # 3. control nets.  The transformer is handed timesteps / 1000 (:734) and feeds its control nets `timestep.to(hidden.dtype) * 1000`
        #    (lightcontrol_flux.py:447, :505): the same value forward_train forms from `t` below
        t = timesteps.to(device=dev, dtype=torch.float32).reshape(B) / 1000
        t1000 = (t.to(torch.bfloat16) * 1000).float().contiguous()
        outs = tr.forward(guided_hint.to(dev), t1000)
        # 4. transformer forward with saves and the control injections
        pred, _ = self.chain.forward_train(st, noisy, t, control=add_control_outputs(outs), keep_head=True)
        self._mark("forward")
        # 5. loss and d noise_pred
        loss, seed = ops.mse_loss_grad(pred, target, grad_scale)
        self._mark("loss head")
        # 6. activation-gradient chain down to injection 0; every net's backward at its injection
        self.chain.backward(seed=seed, on_injection=self._on_injection, stop_after_injections=True)
        self._mark("transformer backward")
        # 7. clip + AdamW
        if optimizer_step:
            tr.step()
            self._mark("optimizer")
        return loss.reshape(())
