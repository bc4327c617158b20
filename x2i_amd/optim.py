"""FlatAdamW: the optimizer half shared by the trainers (ProjectorTrainer in x2i_amd/train.py, ControlNeXtTrainer in x2i_amd/lightcontrol_train.py).

Parameters stay the modules' own bf16 tensors, updated in place; gradients and the two moments are f32 in ONE flat buffer each, in the order the
(name, parameter) pairs were given: a single RCCL all-reduce per step, one global-norm reduction for the clip.  A trainer derives from it, writes its
backward into `g(name)` and overrides `_weights_changed` for the caches it keeps of the weights.

FlatAdamW8bit is the same optimizer half with block-wise 8-bit moments (the reference's --use_8bit_adam, bnb.optim.AdamW8bit): one uint8 code
per element and moment, one f32 absmax per block of 256 elements, every large parameter updated in ONE launch (csrc/optim8.hip; the format is in
DESIGN.md section 4).  `eight_bit(cls)` gives a trainer class its 8-bit variant."""
import functools

import numpy as np
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


BLOCK = 256           # elements per quantisation block; a block never straddles parameters
MIN_8BIT_SIZE = 4096  # parameters with fewer elements keep f32 moments and ops.adamw_ (bitsandbytes' min_8bit_size)


def dynamic_map(signed):
    """The 256 sorted f32 code values of a moment, as a CPU tensor: decade i = 0..6 holds the midpoints of linspace(0.1, 1, k + 1) times
    10^(i - 6), with k = 2^i of both signs (signed, first moment) or k = 2^(i + 1) positive ones (unsigned, second moment); plus 0 and 1.0.
    Signed: 127 negative entries from -0.99296875, zero at index 127, smallest positive 5.5e-7.  Unsigned: zero at index 0, smallest positive
    3.25e-7.  Evaluated in float64, rounded once to f32."""
    vals = [0.0, 1.0]
    for i in range(7):
        edges = np.linspace(0.1, 1.0, 2 ** (i if signed else i + 1) + 1)
        mid = (edges[:-1] + edges[1:]) / 2 * 10.0 ** (i - 6)
        vals += mid.tolist()
        if signed:
            vals += (-mid).tolist()
    vals.sort()
    assert len(vals) == 256
    return torch.tensor(vals, dtype=torch.float64).to(torch.float32)


class FlatAdamW8bit(FlatAdamW):
    """FlatAdamW with block-wise 8-bit moments: same constructor, g / named_grads / zero_grad, _weights_changed hook and step() contract.

    The flat f32 gradient buffer holds the large parameters (>= MIN_8BIT_SIZE elements) first, each on a multiple of BLOCK elements and padded to
    one (the padding stays 0: it changes neither the norm nor the all-reduce), then the small ones back to back.  Block b of the 8-bit state is
    then elements [256 b, 256 b + 256) of the gradient buffer and of the two code arrays, with absmax_m[b] / absmax_v[b]; only the parameter is
    indirect: `table` int64 [blocks, 2] = (address of the block's first element, valid count), built once.  The small parameters keep f32
    moments (`m`, `v`: their region only) and the per-parameter ops.adamw_, bit for bit what FlatAdamW does for them."""

    def __init__(self, named_params, lr, betas, eps, weight_decay, max_grad_norm, process_group=None):
        self.lr, self.betas, self.eps, self.wd, self.max_norm = lr, betas, eps, weight_decay, max_grad_norm
        self.pg = process_group
        self.names, self.params, self.off = [], [], {}
        for n, p in named_params:
            self.names.append(n)
            self.params.append(p)
        self.large = [i for i, p in enumerate(self.params) if p.numel() >= MIN_8BIT_SIZE]
        self.small = [i for i, p in enumerate(self.params) if p.numel() < MIN_8BIT_SIZE]
        o = 0
        for i in self.large:
            self.off[self.names[i]] = (o, self.params[i].numel())
            o += -(-self.params[i].numel() // BLOCK) * BLOCK
        self.blocks, self.small_base = o // BLOCK, o
        for i in self.small:
            self.off[self.names[i]] = (o, self.params[i].numel())
            o += self.params[i].numel()
        dev = self.params[0].device
        self.grad = torch.zeros((o,), device=dev, dtype=torch.float32)
        self.m = torch.zeros((o - self.small_base,), device=dev, dtype=torch.float32)
        self.v = torch.zeros_like(self.m)
        self.code_m = torch.zeros((self.small_base,), device=dev, dtype=torch.uint8)
        self.code_v = torch.zeros_like(self.code_m)
        self.absmax_m = torch.zeros((self.blocks,), device=dev, dtype=torch.float32)   # 0: the state decodes to 0 whatever the codes hold
        self.absmax_v = torch.zeros_like(self.absmax_m)
        self.map_m = dynamic_map(True).to(dev)
        self.map_v = dynamic_map(False).to(dev)
        self._table_ptrs, self.table = None, None
        self._build_table()
        self.step_count = 0
        self.last_norm = None

    def _build_table(self):
        """(address of the block's first parameter element, valid count) per block; rebuilt only if a parameter's storage moved"""
        ptrs = [self.params[i].data_ptr() for i in self.large]
        if ptrs == self._table_ptrs:
            return
        rows = []
        for i, ptr in zip(self.large, ptrs):
            p = self.params[i]
            if p.dtype != torch.bfloat16 or not p.is_contiguous():
                raise ValueError("FlatAdamW8bit: parameter %s must be a contiguous bf16 tensor" % self.names[i])
            n = p.numel()
            rows += [(ptr + 2 * e, min(BLOCK, n - e)) for e in range(0, n, BLOCK)]
        self.table = torch.tensor(rows, dtype=torch.int64).view(-1, 2).to(self.params[0].device)
        self._table_ptrs = ptrs

    def state_bytes(self):
        """bytes of optimizer state held: codes and absmax of the 8-bit blocks (block padding included), the block table, the f32 moments of
        the small parameters.  (The two 1 KiB code maps are constants, not state.)"""
        return sum(t.numel() * t.element_size() for t in (self.code_m, self.code_v, self.absmax_m, self.absmax_v, self.table, self.m, self.v))

    @torch.no_grad()
    def step(self):
        """FlatAdamW.step with the large parameters' update as ONE block-wise 8-bit launch; same return value."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(self.pg) > 1:
            dist.all_reduce(self.grad, group=self.pg)
            ops.reduce_rows(self.grad, self.grad, np_=1, len_=self.grad.numel(), alpha=1.0 / dist.get_world_size(self.pg))
        coef = ops.clip_coef(ops.sum_all(self.grad, squares=True), self.max_norm)
        self.step_count += 1
        kw = dict(lr=self.lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, weight_decay=self.wd, step=self.step_count, coef=coef)
        if self.blocks:
            self._build_table()
            ops.adamw8_(self.table, self.grad, self.code_m, self.code_v, self.absmax_m, self.absmax_v, self.map_m, self.map_v, **kw)
        for i in self.small:
            o, s = self.off[self.names[i]]
            ops.adamw_(self.params[i], self.grad[o:o + s], self.m[o - self.small_base:o - self.small_base + s],
                       self.v[o - self.small_base:o - self.small_base + s], **kw)
        self.grad.zero_()
        self._weights_changed()
        self.last_norm = coef
        return coef


@functools.lru_cache(maxsize=None)
def eight_bit(cls):
    """The 8-bit variant of a trainer class derived from FlatAdamW: the same class with FlatAdamW8bit in front of FlatAdamW in its method
    resolution order, so that its `super().__init__` builds, and its step() runs, the 8-bit optimizer half."""
    return type(cls.__name__ + "8bit", (cls, FlatAdamW8bit), {"__doc__": cls.__doc__})


class EightBitOption:
    """Mixin in front of FlatAdamW in a trainer's bases: the keyword `use_8bit_adam=True` makes the constructor return the trainer's
    eight_bit() variant; with the default the object is the trainer class itself, unchanged."""

    def __new__(cls, *args, use_8bit_adam=False, **kwargs):
        return object.__new__(eight_bit(cls) if use_8bit_adam and not issubclass(cls, FlatAdamW8bit) else cls)
