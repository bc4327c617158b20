"""The MiniCPM-o Resampler without a GPU: the float64 restatement of tests/resampler_ref.py against the reference module's recorded
float64 output (tests/golden/resampler_tiny.safetensors), the position table and ids, the checkers against the mistakes they are there to
catch, the extension header include/x2i_resampler.h (its prototypes against the binding: tests/test_extension_boundary_cpu.py), and the host module's plumbing."""
import ctypes as C
import os

import pytest
import torch
from safetensors import safe_open

from tests import resampler_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "resampler_tiny.safetensors")
RESTATEMENT_BOUND = 1e-10       # both sides float64; they differ in summation order only


@pytest.fixture(scope="module")
def golden():
    with safe_open(FIXTURE, "pt") as f:
        t = {k: f.get_tensor(k) for k in f.keys()}
        meta = {k: int(v) for k, v in f.metadata().items()}
    sd = {k[3:]: v.float() for k, v in t.items() if k.startswith("sd.")}
    sizes = [tuple(s) for s in t["tgt_sizes"].tolist()]
    # the reference's own float32 table where the grids index it, the restatement's elsewhere (never read)
    table = RR.position_table(meta["embed"])
    table[:3, :5] = t["pos_3x5"].double()
    return dict(sd=sd, x=t["x"], sizes=sizes, out=t["out"], meta=meta, table=table, pos_3x5=t["pos_3x5"], pos_2x2=t["pos_2x2"])


# ---------------------------------------------------------------------------------------------------------------- the restatement
def test_fixture_is_what_the_generator_says(golden):
    m = golden["meta"]
    assert m == dict(embed=256, heads=2, kv_dim=64, queries=8) and golden["sizes"] == [(3, 5), (2, 2)]
    assert golden["out"].dtype == torch.float64 and golden["out"].shape == (2, 8, 256) and golden["x"].shape == (2, 15, 64)
    assert os.path.getsize(FIXTURE) < 1 << 20
    assert torch.equal(golden["pos_2x2"], golden["pos_3x5"][:2, :2])
    want = RR.random_state_dict(8, 256, 64, 20)
    assert set(want) == set(golden["sd"]) and all(torch.equal(want[k], v) for k, v in golden["sd"].items())


def test_float64_restatement_meets_the_reference_output(golden):
    got = RR.module_reference(golden["sd"], golden["x"], golden["sizes"], num_heads=2, table=golden["table"])
    e = RR.rel_l2(got, golden["out"])
    print("float64 restatement against the reference module in float64: rel-L2 %.3e (bound %.0e)" % (e, RESTATEMENT_BOUND))
    assert e <= RESTATEMENT_BOUND
    # ... and with the restatement's own table, which may differ from the recorded one in float32's last place
    own = RR.rel_l2(RR.module_reference(golden["sd"], golden["x"], golden["sizes"], num_heads=2), golden["out"])
    print("with the restatement's own position table: rel-L2 %.3e" % own)
    assert own <= 1e-6


def test_padding_rows_of_x_reach_nothing(golden):
    x2 = golden["x"].clone()
    x2[1, 4:] = 1000.0
    a = RR.module_reference(golden["sd"], golden["x"], golden["sizes"], num_heads=2, table=golden["table"])
    b = RR.module_reference(golden["sd"], x2, golden["sizes"], num_heads=2, table=golden["table"])
    assert torch.equal(a, b)


def test_the_module_checker_rejects_planted_errors(golden):
    sd, x, sizes, out = golden["sd"], golden["x"], golden["sizes"], golden["out"]
    one_more = RR.rel_l2(RR.module_reference(sd, x, sizes, num_heads=2, table=golden["table"], fault="one_more"), out)
    swapped = RR.rel_l2(RR.module_reference(sd, x, sizes, num_heads=2, table=RR.position_table(256, fault="swap")), out)
    print("planted errors: one key too many %.3e, swapped sin/cos %.3e" % (one_more, swapped))
    assert one_more > 1e-3 and swapped > 1e-3


# ---------------------------------------------------------------------------------------------------------------- position table and ids
def test_position_table_against_the_references_slices(golden):
    from x2i_amd.resampler import sincos_table
    mine, ref = sincos_table(256), RR.position_table(256)
    assert mine.dtype == torch.float32 and mine.shape == (70, 70, 256)
    for t in (mine.double(), ref):
        assert float((t[:3, :5] - golden["pos_3x5"].double()).abs().max()) <= 1e-6
        assert float((t[:2, :2] - golden["pos_2x2"].double()).abs().max()) <= 1e-6
    assert float((mine.double() - ref).abs().max()) <= 1e-6
    # the layout: the first half of the channels follows the column, the second the row; sin before cos (sin 0 = 0, cos 0 = 1)
    assert torch.equal(mine[5, 0, :64], torch.zeros(64)) and torch.equal(mine[5, 0, 64:128], torch.ones(64))
    assert torch.equal(mine[0, 5, 128:192], torch.zeros(64)) and torch.equal(mine[0, 5, 192:], torch.ones(64))
    assert torch.equal(mine[7, 3, :128], mine[0, 3, :128]) and torch.equal(mine[7, 3, 128:], mine[7, 0, 128:])
    assert abs(float(mine[0, 1, 0]) - 0.8414709848) < 1e-6 and abs(float(mine[1, 0, 192]) - 0.5403023059) < 1e-6
    # the planted error is seen
    assert float((RR.position_table(256, fault="swap")[:3, :5] - golden["pos_3x5"].double()).abs().max()) > 0.1
    with pytest.raises(ValueError, match="embed_dim % 4"):
        sincos_table(130)


@pytest.mark.parametrize("h,w", [(3, 5), (32, 32), (20, 27), (1, 1)])
def test_position_ids(h, w):
    from x2i_amd.resampler import position_ids
    L = h * w + 3
    got = position_ids([(h, w), (1, 1)], L)
    assert got.dtype == torch.int32 and got.shape == (2, L)
    assert torch.equal(got.long(), RR.position_ids([(h, w), (1, 1)], L))
    rows, cols = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    assert torch.equal(got[0, :h * w].long(), (rows * 70 + cols).flatten())
    assert bool((got[0, h * w:] == -1).all()) and got[1].tolist() == [0] + [-1] * (L - 1)
    assert int(got.max()) == (h - 1) * 70 + w - 1


# ---------------------------------------------------------------------------------------------------------------- the kernel checkers
def test_attention_reference_masks_by_count_and_the_checker_sees_one_key_too_many():
    g = torch.Generator().manual_seed(5)
    Q = torch.randn((2, 8, 128), generator=g)
    K, V = torch.randn((3, 2, 20, 128), generator=g), torch.randn((3, 2, 20, 128), generator=g)
    n = [20, 7, 0]
    ref = RR.attention_reference(Q, K, V, n, 128 ** -0.5)
    assert ref.shape == (3, 2, 8, 128) and not bool(ref[2].any())
    # sample 1 is the attention over its first 7 keys alone; what lies beyond them is never read
    K2, V2 = K.clone(), V.clone()
    K2[1, :, 7:], V2[1, :, 7:] = float("nan"), float("nan")
    assert torch.equal(RR.attention_reference(Q, K2, V2, n, 128 ** -0.5), ref)
    alone = RR.attention_reference(Q, K[1:2, :, :7], V[1:2, :, :7], None, 128 ** -0.5)
    assert RR.rel_l2(alone[0], ref[1]) < 1e-14
    # counts are clamped into [0, L]
    assert torch.equal(RR.attention_reference(Q, K, V, [27, 7, -3], 128 ** -0.5), ref)
    RR.check_attention("self", ref, ref)
    bad = RR.attention_reference(Q, K, V, n, 128 ** -0.5, fault="one_more")
    assert torch.equal(bad[0], ref[0])
    with pytest.raises(AssertionError, match=r"b=1"):
        RR.check_attention("one key too many", bad[:2], ref[:2])
    with pytest.raises(AssertionError, match=r"b=2"):      # an empty sample's zeros must be met exactly
        RR.check_attention("one key too many", bad, ref)


def test_ln_pos_reference():
    g = torch.Generator().manual_seed(6)
    x, w, b = torch.randn((5, 16), generator=g), torch.randn(16, generator=g), torch.randn(16, generator=g)
    pos = torch.randn((4, 16), generator=g)
    xv, xk = RR.ln_pos(x, w, b, 1e-6, [0, 3, -1, 9, -7], pos)
    want = torch.nn.functional.layer_norm(x.double(), (16,), w.double(), b.double(), 1e-6)
    assert RR.rel_l2(xv, want) < 1e-14
    assert torch.equal(xk[2], xv[2]) and torch.equal(xk[4], xv[4]) and torch.equal(xk[3], xv[3] + pos[3].double()) and torch.equal(xk[0], xv[0] + pos[0].double())


def test_library_comparator_agrees_with_the_restatement_in_float64(golden):
    lib = RR.LibraryResampler(8, 256, 2, 64)
    lib.load_state_dict(golden["sd"], strict=True)
    got = lib.double()(golden["x"].double(), golden["sizes"])
    assert RR.rel_l2(got, golden["out"]) < 1e-6       # (its table is the restatement's own)


# ---------------------------------------------------------------------------------------------------------------- boundary
def test_entry_points_validate_their_arguments_without_a_gpu():
    from x2i_amd import resampler_ops
    lib = resampler_ops.load()
    fake, odd = C.c_void_p(0x1000), C.c_void_p(0x1008)  # never dereferenced: validation fails first
    err = lambda: lib.x2i_last_error()
    att = lambda **kw: lib.x2i_resampler_attention_bf16(*[kw.get(k, d) for k, d in (
        ("Q", fake), ("K", fake), ("VT", fake), ("n", None), ("O", fake), ("B", 2), ("H", 2), ("NQ", 64), ("L", 200), ("Lpad", 256),
        ("scale", 128 ** -0.5), ("ldo", 256), ("obs", 64 * 256), ("st", None))])
    assert att(NQ=0) < 0 and b"NQ=0" in err()
    assert att(NQ=65) < 0 and b"NQ=65" in err()
    assert att(Lpad=200) < 0 and b"Lpad" in err()
    assert att(Lpad=192) < 0 and att(L=0) < 0 and att(B=0) < 0 and att(H=0) < 0
    for s in (0.0, -1.0, float("inf"), float("nan")):
        assert att(scale=s) < 0 and b"scale" in err()
    assert att(ldo=248) < 0 and b"128*H" in err()
    assert att(ldo=260) < 0 and att(obs=64 * 256 + 4) < 0
    for k in ("Q", "K", "VT", "O"):
        assert att(**{k: None}) < 0 and b"null" in err()
        assert att(**{k: odd}) < 0 and b"aligned" in err()
    assert att(n=C.c_void_p(0x1002)) < 0 and b"aligned" in err()
    ln = lambda **kw: lib.x2i_resampler_ln_pos_bf16(*[kw.get(k, d) for k, d in (
        ("X", fake), ("ldx", 256), ("w", fake), ("b", fake), ("eps", 1e-6), ("ids", fake), ("pos", fake), ("n_pos", 4900), ("XV", C.c_void_p(0x100000)),
        ("ldv", 256), ("XK", C.c_void_p(0x200000)), ("ldk", 256), ("rows", 77), ("D", 256), ("st", None))])
    assert ln(D=252, ldx=252) < 0 and b"D=252" in err()
    assert ln(D=4104, ldx=4104, ldv=4104, ldk=4104) < 0 and ln(D=0) < 0 and ln(rows=0) < 0 and ln(n_pos=0) < 0
    assert ln(ldx=248) < 0 and ln(ldv=248) < 0 and ln(ldk=260) < 0 and b"strides" in err()
    assert ln(eps=-1.0) < 0 and b"eps" in err()
    for k in ("X", "w", "b", "ids", "pos", "XV", "XK"):
        assert ln(**{k: None}) < 0 and b"null" in err()
    for k in ("X", "w", "b", "pos", "XV", "XK"):
        assert ln(**{k: C.c_void_p(0x300008)}) < 0 and b"aligned" in err()
    assert ln(ids=C.c_void_p(0x1002)) < 0
    assert ln(XV=fake) < 0 and b"alias" in err()
    assert ln(XK=C.c_void_p(0x1000 + 2 * 256 * 10)) < 0 and b"alias" in err()      # inside X's rows
    assert ln(XK=C.c_void_p(0x100000)) < 0 and b"alias" in err()                   # XV is XK
    split = lambda **kw: lib.x2i_resampler_kv_split_bf16(*[kw.get(k, d) for k, d in (
        ("Kr", fake), ("ldk", 512), ("Vr", fake), ("ldv", 512), ("K", fake), ("VT", fake), ("B", 1), ("L", 81), ("Lpad", 128), ("H", 2), ("st", None))])
    assert split(ldk=248) < 0 and b"128*H" in err()
    assert split(ldv=516) < 0 and split(Lpad=80) < 0 and split(Lpad=84) < 0 and split(H=0) < 0 and split(H=70000) < 0 and split(B=0) < 0 and split(L=0) < 0
    for k in ("Kr", "Vr", "K", "VT"):
        assert split(**{k: None}) < 0 and b"null" in err()
        assert split(**{k: odd}) < 0 and b"aligned" in err()


# ---------------------------------------------------------------------------------------------------------------- host module
def _tiny(**kw):
    from x2i_amd.resampler import Resampler
    f = dict(num_queries=8, embed_dim=256, kv_dim=64, device="cpu")
    f.update(kw)
    return Resampler(**f)


def test_unsupported_configurations_raise():
    for bad, msg in ((dict(dtype=torch.float32), "bf16"), (dict(embed_dim=192), "heads of 128"), (dict(num_heads=4), "heads of 128"),
                     (dict(num_queries=0), "queries"), (dict(num_queries=65), "queries"), (dict(kv_dim=256), "kv_dim"), (dict(kv_dim=None), "kv_dim")):
        with pytest.raises(ValueError, match=msg):
            _tiny(**bad)
    with pytest.raises(ValueError, match="bf16"):
        _tiny().float()


def test_parameter_names_are_the_references_and_the_caches_follow_the_module(golden):
    m = _tiny()
    assert set(m.state_dict()) == set(golden["sd"]) and all(m.state_dict()[k].shape == v.shape for k, v in golden["sd"].items())
    assert m._projT is None and m._Q is None
    m.load_state_dict({k: v.bfloat16() for k, v in golden["sd"].items()}, strict=True)
    assert all(torch.equal(v.float(), golden["sd"][k]) for k, v in m.state_dict().items())
    assert torch.equal(m._projT, m.proj.t()) and m._projT.is_contiguous()
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in golden["sd"].items() if k != "ln_kv.bias"}, strict=True)
    # the cached Q is dropped when the parameters may have changed
    for change in (lambda: m.pack_(), lambda: m.to(torch.bfloat16), lambda: m.load_state_dict({k: v.bfloat16() for k, v in golden["sd"].items()})):
        m._Q = "stale"
        change()
        assert m._Q is None
    before = m._projT
    m.proj.mul_(2.0)
    assert m.pack_()._projT is not before and torch.equal(m._projT, m.proj.t())
    # the position table is the float32 table rounded once, and no parameter
    assert m._pos.dtype == torch.bfloat16 and m._pos.shape == (4900, 256) and "_pos" not in m.state_dict()
    from x2i_amd.resampler import sincos_table
    assert torch.equal(m._pos, sincos_table(256).bfloat16().reshape(4900, 256))
    # from_hf copies an instantiated module
    lib = RR.LibraryResampler(8, 256, 2, 64)
    lib.load_state_dict(golden["sd"], strict=True)
    from x2i_amd.resampler import Resampler
    copy = Resampler.from_hf(lib)
    assert (copy.num_queries, copy.embed_dim, copy.num_heads, copy.kv_dim) == (8, 256, 2, 64) and copy.device.type == "cpu"
    assert all(torch.equal(v.float(), golden["sd"][k]) for k, v in copy.state_dict().items())


def test_plan_holds_ids_counts_and_refuses_what_the_table_cannot_reach():
    m = _tiny()
    p = m.plan(torch.tensor([(3, 5), (2, 2)]), 15)
    assert p.sizes == ((3, 5), (2, 2)) and (p.B, p.L, p.Lpad) == (2, 15, 64)
    assert p.n_keys.dtype == torch.int32 and p.n_keys.tolist() == [15, 4]
    assert p.ids.dtype == torch.int32 and torch.equal(p.ids.long(), RR.position_ids([(3, 5), (2, 2)], 15).reshape(-1))
    assert not hasattr(p, "ws")        # workspaces live on the GPU only
    for bad, msg in (([(71, 1)], "position table"), ([(1, 71)], "position table"), ([(4, 4)], "h \\* w <= L"), ([(0, 3)], "positive"), ([], "tgt_sizes")):
        with pytest.raises(ValueError, match=msg):
            m.plan(bad, 15 if bad != [(71, 1)] and bad != [(1, 71)] else 71)
    with pytest.raises(ValueError, match="runs on the GPU only"):
        m(torch.zeros((2, 15, 64)), plan=p)
    with pytest.raises(ValueError, match="kv_dim"):
        m(torch.zeros((2, 15, 32)), tgt_sizes=torch.tensor([(3, 5), (2, 2)]))
    with pytest.raises(ValueError, match="tgt_sizes"):
        m(torch.zeros((2, 15, 64)))
