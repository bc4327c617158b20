"""The host plumbing that the HIP encoder modules share: T5Stack, CLIPTextModel, Qwen2DecoderStack, Qwen2_5VisionTower, SiglipVisionTower,
WhisperAudioTower, InternVisionTower, InternVLVision and Resampler derive from PackedModule.

A module's kernels read three kinds of tensors: ordinary parameters, FUSED storage (`_fused[name]`: stacked or zero-padded matrices, of
which some parameters are views, so that a checkpoint's keys load strictly into the layout the GEMMs want) and DERIVED COPIES that a
subclass's pack_() makes of parameters (a head-padded, permuted, transposed or f32 copy is no view).  The one rule that keeps the three in
step lives here, in _apply and load_state_dict:
    move the fused storage, re-point the views, drop the caches, move the parameters, re-make the copies.
A view that is not re-pointed after .to(), or a copy that is not re-made after a load, runs the kernels on stale weights without a word.

flux.py, vae.py and lightcontrol.py are not built on this: FluxTransformer's _apply re-quantises fp8 weights and does not go through
nn.Module._apply, and the other two pack per convolution.
"""
import copy

import torch
import torch.nn as nn


class WB(nn.Module):
    """A `.weight` and, with one, a `.bias`: what the libraries' Linear, LayerNorm, Embedding and Conv modules are to a state dict"""

    def __init__(self, weight, bias=None):
        super().__init__()
        as_param = lambda t: t if isinstance(t, nn.Parameter) else nn.Parameter(t, requires_grad=False)
        self.weight = as_param(weight)
        if bias is not None:
            self.bias = as_param(bias)


def config_fields(defaults, config, kw, who, extra=None):
    """The fields of `defaults` as a dict: each from `config` where it has one, then from kw; a kw that is no field is a TypeError.
    extra(config) -> fields that the library's config spells differently (Qwen's rope parameters)."""
    f = dict(defaults)
    if config is not None:
        for k in f:
            f[k] = getattr(config, k, f[k])
        if extra is not None:
            f.update(extra(config))
    unknown = set(kw) - set(f)
    if unknown:
        raise TypeError("%s: unknown configuration fields %s" % (who, sorted(unknown)))
    f.update(kw)
    return f


def config_object(name, fields):
    """The `.config` of a module: an object of a class called `name` with the fields as attributes"""
    return type(name, (), dict(fields))()


class PackedModule(nn.Module):
    """bf16 parameters, fused storage with parameter views, derived copies and per-shape caches (the module docstring).  The constructor
    registers nothing, so a subclass's parameters come in the order it creates them."""

    _eval_only = False      # True: train(True) raises
    _copies = None          # the attribute that holds what pack_() makes (None before the first pack_()), if the subclass has a pack_()

    def __init__(self, device=None):
        super().__init__()
        self._build_device = None if device is None else torch.device(device)    # where _store and _param allocate; `device` is where it is now
        self._fused = {}        # name -> bf16 tensor
        self._views = []        # (parameter, fused name, index, shape or None)
        self._ws = {}           # workspaces of the resident (B, S)
        self._plans = {}        # the resident plan

    # ------------------------------------------------------------------ storage
    def _store(self, name, *shape, zero=False):
        self._fused[name] = (torch.zeros if zero else torch.empty)(shape, device=self._build_device, dtype=torch.bfloat16)
        return self._fused[name]

    def _param(self, *shape):
        return nn.Parameter(torch.empty(shape, device=self._build_device, dtype=torch.bfloat16), requires_grad=False)

    def _view(self, name, index, shape=None):
        """A parameter that is _fused[name][index], reshaped to `shape` if given"""
        t = self._fused[name][index]
        p = nn.Parameter(t if shape is None else t.view(shape), requires_grad=False)
        self._views.append((p, name, index, shape))
        return p

    # ------------------------------------------------------------------ nn.Module plumbing
    @property
    def dtype(self):
        return torch.bfloat16

    @property
    def device(self):
        for t in self._fused.values():
            return t.device
        return next(self.parameters()).device

    def train(self, mode=True):
        if mode and self._eval_only:
            raise ValueError("x2i_amd %s is eval-only" % type(self).__name__)
        return super().train(mode)

    def _bf16(self, t):
        if t.dtype != torch.bfloat16:
            raise ValueError("x2i_amd %s is bf16-only" % type(self).__name__)
        return t

    def _moved(self, fn):
        """What a subclass caches beyond _ws and _plans is dropped, or moved through fn (self._bf16(fn(t))), here"""
        self._ws, self._plans = {}, {}

    def _repoint(self):
        for p, name, index, shape in self._views:
            t = self._fused[name][index]
            p.data = t if shape is None else t.view(shape)

    def __deepcopy__(self, memo):
        # copying a Parameter clones its data, which would leave the copy's views with storage of their own (values equal, writes unseen)
        new = type(self).__new__(type(self))
        memo[id(self)] = new
        new.__setstate__(copy.deepcopy(self.__dict__, memo))
        new._repoint()
        return new

    def _apply(self, fn, recurse=True):
        moved = {k: self._bf16(fn(t)) for k, t in self._fused.items()}      # every one checked before any is replaced
        self._fused.update(moved)
        self._repoint()
        packed = self._copies is not None and getattr(self, self._copies) is not None
        self._moved(fn)
        out = super()._apply(fn, recurse)
        if packed:
            self.pack_()
        return out

    def _canonical_keys(self, state_dict):
        return state_dict

    def load_state_dict(self, state_dict, strict=True, assign=False):
        if assign and any(getattr(m, "_views", None) for m in self.modules()):
            raise ValueError("x2i_amd %s: assign=True would detach the parameters that are views of fused storage" % type(self).__name__)
        out = super().load_state_dict(self._canonical_keys(state_dict), strict=strict, assign=assign)
        self.pack_()
        return out

    def pack_(self):
        """Makes the derived copies again from the parameters as they are now (after they were written in place); none here"""
        return self

    # ------------------------------------------------------------------ caches and tools
    def _plan_for(self, *key):
        """self.plan(*key), with the plan of the last key kept"""
        p = self._plans.get(key)
        if p is None:
            p = self.plan(*key)
            self._plans = {key: p}      # keep one shape resident
        return p

    @torch.no_grad()
    def _init_random(self, seed, rule, root=None):
        """One N(0, 1) draw r per parameter of `root` (default: self) in named_parameters() order, written as rule(name, parameter, r)"""
        gen = torch.Generator(device=self.device).manual_seed(seed)
        for n, p in (self if root is None else root).named_parameters():
            r = torch.randn(p.shape, device=p.device, generator=gen)
            p.copy_(rule(n, p, r))
