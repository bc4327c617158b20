"""The contract of x2i_amd._packed.PackedModule, on a toy subclass: what the nine encoder modules rely on when a checkpoint is loaded, the
module is copied (handoff deep-copies) or moved (.to): views follow the fused storage, derived copies are made again, caches are dropped."""
import copy

import pytest
import torch

from x2i_amd._packed import WB, PackedModule, config_fields, config_object


class Toy(PackedModule):
    """fused "w" [6, 8]: rows 0:2 and 2:4 are two row-slice views, rows 4:6 x columns 0:6 a reshaped [2, 2, 3] view (columns 6:8 stay zero);
    fused "z" [4]: a bias view; `lin` an ordinary parameter; pack_() makes lin's transposed copy"""
    _copies = "_linT"

    def __init__(self):
        super().__init__("cpu")
        self._store("w", 6, 8, zero=True)
        self._store("z", 4)
        self.a = WB(self._view("w", slice(0, 2)), self._view("z", slice(0, 2)))
        self.b = WB(self._view("w", slice(2, 4)))
        self.conv = WB(self._view("w", (slice(4, 6), slice(0, 6)), (2, 2, 3)))
        self.lin = self._param(3, 5)
        self._linT = None
        self.packs = 0

    def pack_(self):
        self.packs += 1
        self._linT = self.lin.t().contiguous()
        return self

    def plan(self, B, S):
        return [B, S]

    def init_random_(self, seed=0):
        self._init_random(seed, lambda n, p, r: 0.1 * r if p.dim() == 1 else r * p.shape[-1] ** -0.5)
        return self.pack_()


VIEWS = (("a.weight", "w", lambda f: f[0:2]), ("a.bias", "z", lambda f: f[0:2]), ("b.weight", "w", lambda f: f[2:4]),
         ("conv.weight", "w", lambda f: f[4:6, 0:6]))


def mover():
    """The CPU stand-in of .to("cuda"): a tensor of the old world is cloned; one that already moved comes back as it is, as Tensor.to does"""
    new = set()

    def fn(t):
        if t.untyped_storage().data_ptr() in new:
            return t
        c = t.clone()
        new.add(c.untyped_storage().data_ptr())
        return c
    return fn


def assert_views_alias(m):
    sd = dict(m.named_parameters())
    for key, name, index in VIEWS:
        assert sd[key].data_ptr() == index(m._fused[name]).data_ptr(), key
        assert sd[key].untyped_storage().data_ptr() == m._fused[name].untyped_storage().data_ptr(), key
    assert sd["conv.weight"].shape == (2, 2, 3) and sd["lin"].untyped_storage().data_ptr() not in {t.untyped_storage().data_ptr() for t in m._fused.values()}


def test_registration_order_is_the_subclasss_and_the_base_registers_nothing():
    assert list(PackedModule().state_dict()) == [] and list(PackedModule().buffers()) == []
    m = Toy()
    assert list(m.state_dict()) == ["lin", "a.weight", "a.bias", "b.weight", "conv.weight"]
    assert m.dtype == torch.bfloat16 and m.device.type == "cpu" and m._linT is None and m.packs == 0
    assert_views_alias(m)
    assert not bool(m._fused["w"][:, 6:].any())


def test_deepcopy_views_alias_the_copys_own_storage():
    m = Toy().init_random_(1)
    c = copy.deepcopy(m)
    assert_views_alias(c)
    assert c._fused["w"].untyped_storage().data_ptr() != m._fused["w"].untyped_storage().data_ptr()
    assert all(torch.equal(v, m.state_dict()[k]) for k, v in c.state_dict().items()) and torch.equal(c._linT, m._linT) and c._linT is not m._linT
    with torch.no_grad():
        c.b.weight.fill_(3.0)
        c.conv.weight.fill_(5.0)
    assert bool((c._fused["w"][2:4] == 3.0).all()) and bool((c._fused["w"][4:6, :6] == 5.0).all()) and not bool(c._fused["w"][4:6, 6:].any())
    assert not bool((m._fused["w"][2:4] == 3.0).any())


def test_apply_moves_storage_repoints_views_drops_caches_and_packs_again():
    m = Toy().init_random_(2)
    want = {k: v.clone() for k, v in m.state_dict().items()}
    old = {t.untyped_storage().data_ptr() for t in m._fused.values()} | {m.lin.untyped_storage().data_ptr()}
    before, packs = m._linT, m.packs
    m._plan_for(2, 3)
    m._ws = {(2, 3): "stale"}
    assert m._apply(mover()) is m
    assert_views_alias(m)
    assert not old & {p.untyped_storage().data_ptr() for p in m.parameters()}
    assert not old & {t.untyped_storage().data_ptr() for t in m._fused.values()}
    assert all(torch.equal(v, want[k]) for k, v in m.state_dict().items())
    assert m._linT is not before and torch.equal(m._linT, before) and m.packs == packs + 1
    assert m._plans == {} and m._ws == {}


def test_another_dtype_is_refused_before_any_storage_is_replaced():
    m = Toy().init_random_(3)
    fused = dict(m._fused)
    ptrs = {k: p.data_ptr() for k, p in m.named_parameters()}
    with pytest.raises(ValueError, match="x2i_amd Toy is bf16-only"):
        m.float()
    # the first fused tensor converts, the second does not: nothing of the first may have been kept
    with pytest.raises(ValueError, match="bf16-only"):
        m._apply(lambda t: t.float() if t is fused["z"] else t.clone())
    assert all(m._fused[k] is t and t.dtype == torch.bfloat16 for k, t in fused.items()) and list(m._fused) == list(fused)
    assert {k: p.data_ptr() for k, p in m.named_parameters()} == ptrs and all(p.dtype == torch.bfloat16 for p in m.parameters())
    assert_views_alias(m)


def test_load_state_dict_refuses_assign_is_strict_and_packs_once():
    m, src = Toy().init_random_(4), Toy().init_random_(5)
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    want = {k: v.clone() for k, v in m.state_dict().items()}
    packs = m.packs
    with pytest.raises(ValueError, match="assign"):
        m.load_state_dict(sd, assign=True)
    assert all(torch.equal(v, want[k]) for k, v in m.state_dict().items()) and m.packs == packs
    assert_views_alias(m)
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != "b.weight"}, strict=True)
    packs = m.packs
    m.load_state_dict(sd, strict=True)
    assert m.packs == packs + 1 and all(torch.equal(v, sd[k]) for k, v in m.state_dict().items()) and torch.equal(m._linT, src._linT)
    assert_views_alias(m)
    assert torch.equal(m._fused["w"][0:2], sd["a.weight"]) and torch.equal(m._fused["w"][4:6, :6].reshape(2, 2, 3), sd["conv.weight"])

    class Renamed(Toy):
        def _canonical_keys(self, state_dict):
            return {k[len("model."):]: v for k, v in state_dict.items()}
    r = Renamed()
    r.load_state_dict({"model." + k: v for k, v in sd.items()}, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in r.state_dict().items())

    class NoViews(PackedModule):
        def __init__(self):
            super().__init__("cpu")
            self.w = self._param(2, 2)
    n = NoViews()
    t = torch.ones((2, 2), dtype=torch.bfloat16)
    n.load_state_dict({"w": t}, assign=True)          # nothing to detach: assign is forwarded
    assert n.w.data_ptr() == t.data_ptr() and n.device.type == "cpu"


def test_a_module_never_packed_is_not_packed_by_apply():
    m = Toy()
    m._apply(mover())
    assert m.packs == 0 and m._linT is None
    assert_views_alias(m)
    m.to(torch.bfloat16)
    assert m.packs == 0


def test_plan_for_keeps_one_plan():
    m = Toy()
    p = m._plan_for(2, 3)
    assert p == [2, 3] and m._plan_for(2, 3) is p and list(m._plans) == [(2, 3)]
    q = m._plan_for(1, 3)
    assert list(m._plans) == [(1, 3)] and m._plan_for(1, 3) is q and m._plan_for(2, 3) is not p


def test_init_random_draws_once_per_parameter_in_order(monkeypatch):
    a, b = Toy().init_random_(7), Toy().init_random_(7)
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items()) and torch.equal(a._fused["w"], b._fused["w"])
    assert not torch.equal(a.lin, Toy().init_random_(8).lin)
    # the loop, by hand
    c = Toy()
    gen = torch.Generator(device="cpu").manual_seed(7)
    with torch.no_grad():
        for n, p in c.named_parameters():
            r = torch.randn(p.shape, device=p.device, generator=gen)
            p.copy_(0.1 * r if p.dim() == 1 else r * p.shape[-1] ** -0.5)
    assert all(torch.equal(v, a.state_dict()[k]) for k, v in c.state_dict().items())
    drawn, randn = [], torch.randn
    monkeypatch.setattr(torch, "randn", lambda shape, **kw: drawn.append(tuple(shape)) or randn(shape, **kw))
    d = Toy().init_random_(7)
    assert drawn == [tuple(p.shape) for _, p in d.named_parameters()] and len(drawn) == 5
    assert all(torch.equal(v, a.state_dict()[k]) for k, v in d.state_dict().items())
    # another root: the parameters of a child alone
    drawn.clear()
    d._init_random(1, lambda n, p, r: r, root=d.a)
    assert drawn == [(2, 8), (2,)]


def test_eval_only_flag_and_config_fields():
    class Frozen(Toy):
        _eval_only = True
    f = Frozen()
    assert f.eval() is f and not f.training
    with pytest.raises(ValueError, match="x2i_amd Frozen is eval-only"):
        f.train()
    assert Toy().train().training
    defaults = dict(width=8, depth=2, theta=1.0)
    lib = config_object("LibConfig", dict(width=16, other=3))
    assert config_fields(defaults, None, {}, "Toy") == defaults and config_fields(defaults, None, {}, "Toy") is not defaults
    assert config_fields(defaults, lib, dict(depth=4), "Toy") == dict(width=16, depth=4, theta=1.0)
    assert config_fields(defaults, lib, {}, "Toy", extra=lambda c: dict(theta=float(c.other))) == dict(width=16, depth=2, theta=3.0)
    assert config_fields(defaults, None, {}, "Toy", extra=lambda c: dict(theta=2.0))["theta"] == 1.0       # no config: nothing to translate
    with pytest.raises(TypeError, match="Toy: unknown configuration fields \\['heads'\\]"):
        config_fields(defaults, lib, dict(heads=2), "Toy")
    c = config_object("ToyConfig", defaults)
    assert type(c).__name__ == "ToyConfig" and (c.width, c.depth) == (8, 2)
