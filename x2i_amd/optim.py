"""FlatAdamW: the optimizer half shared by the trainers (ProjectorTrainer in x2i_amd/train.py, ControlNeXtTrainer in x2i_amd/lightcontrol_train.py).

Parameters stay the modules' own bf16 tensors, updated in place; gradients and the two moments are f32 in ONE flat buffer each, in the order the
(name, parameter) pairs were given: a single RCCL all-reduce per step, one global-norm reduction for the clip.  A trainer derives from it, writes its
backward into `g(name)` and overrides `_weights_changed` for the caches it keeps of the weights."""
import torch

from . import ops


class FlatAdamW:
    def __init__(self, named_params, lr, betas, eps, weight_decay, max_grad_norm, process_group=None):
        self.lr, self.betas, self.eps, self.wd, self.max_norm = lr, betas, eps, weight_decay, max_grad_norm
        self.pg = process_group
        self.names, self.params, self.off = [], [], {}
        o = 0
        for n, p in named_params:
            self.names.append(n)
            self.params.append(p)
            self.off[n] = (o, p.numel())
            o += p.numel()
        self.grad = torch.zeros((o,), device=self.params[0].device, dtype=torch.float32)
        self.m = torch.zeros_like(self.grad)
        self.v = torch.zeros_like(self.grad)
        self.step_count = 0
        self.last_norm = None

    def g(self, name):
        o, s = self.off[name]
        return self.grad[o:o + s]

    def named_grads(self):
        """{parameter name: f32 gradient shaped like the parameter}"""
        return {n: self.g(n).view(p.shape) for n, p in zip(self.names, self.params)}

    def zero_grad(self):
        self.grad.zero_()

    def _weights_changed(self):
        """Called by step() after the update: drop whatever the trainer or its modules cache of the weights.  Host-side only (step() runs next to
        captured graphs: no synchronisation here)."""

    @torch.no_grad()
    def step(self):
        """all-reduce (mean) over the data-parallel group, clip by the global norm of all gradients, AdamW; clears the gradients and every cache
        derived from the weights.  Returns the device tensor [clip coefficient, gradient norm]."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(self.pg) > 1:
            dist.all_reduce(self.grad, group=self.pg)  # one flat buffer: a single RCCL ring all-reduce per step
            ops.reduce_rows(self.grad, self.grad, np_=1, len_=self.grad.numel(), alpha=1.0 / dist.get_world_size(self.pg))  # in place: mean
        coef = ops.clip_coef(ops.sum_all(self.grad, squares=True), self.max_norm)
        self.step_count += 1
        for n, p in zip(self.names, self.params):
            o, s = self.off[n]
            ops.adamw_(p, self.grad[o:o + s], self.m[o:o + s], self.v[o:o + s], lr=self.lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps,
                       weight_decay=self.wd, step=self.step_count, coef=coef)
        self.grad.zero_()
        self._weights_changed()
        self.last_norm = coef
        return coef
