"""Every norm, embedding and update launch of a bf16 denoise step, at the model's geometry, against the float64 reference of tests/ew_ref.py
-- every output element of every launch, and the sentinel outside what the launch may write.

The launch list is taken from the model: a full-width FluxTransformer2DModel (D = 3072, H = 24, guidance_embeds=True) with one double and one
single block, X2I_QKV_FUSE=0 (so that x2i_qkv_split_bf16 serves the QKV split) and a forward hook on every block's attn (so that the
attention outputs are materialised and x2i_gated_residual_bf16 adds them), runs prepare_conditioning, one denoise and prepare_modulation with
ops.ln_modulate / skinny_linear / gated_residual_ / qkv_split / timestep_sinusoid replaced by a recorder.  Each recorded launch is replayed
through the same ops call with the recorded geometry (every shape, stride, offset, S0, mod_bs, ldy; the storages shared as the model shares
them) on fresh storages of each operand kind; outputs start as the sentinel, the RoPE tables are the model's.

Configurations (B, image side), St = 512: (1, 512) -- every LN launch takes ln_kernel (B S = 1536, norm_out 1024 rows); (1, 1024) and
(4, 1024) -- ln_rows_kernel<6, 4>; (2, 1008) -- S = 4481: 4-row waves straddle the samples.  Unit launches cover what the 1 + 1-block model
cannot reach: the full-depth modulation table (N = 344 D), ragged N around the rpw switch at 65536, skinny launches of 1 .. 16 samples
(bit-identical per sample however many share the launch), LayerNorm with ragged S / S0 / row counts and padded strides, the Euler step's
tail kernel.  The largest share of the f32 allowance used per launch is printed (WORST)."""
import inspect
import time

import pytest
import torch

from tests import ew_ref as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
ST = 512
D = 3072
CONFIGS = {"b1_512": (1, 512), "b1_1024": (1, 1024), "b4_1024": (4, 1024), "b2_1008": (2, 1008)}
WRAPPED = ("ln_modulate", "skinny_linear", "gated_residual_", "qkv_split", "timestep_sinusoid")
KINDS = {"ln_modulate": E.LN_KINDS, "skinny_linear": E.SK_KINDS, "gated_residual_": ("random", "outlier"),
         "qkv_split": ("random", "outlier"), "timestep_sinusoid": ("random", "bf16_grid", "edge")}
WORST = {}      # launch -> worst share of the f32 allowance used, over everything this module ran


@pytest.fixture(scope="module")
def ops():
    from x2i_amd import ops as o
    o._lib.load()
    return o


def note(name, share):
    WORST[name] = max(WORST.get(name, 0.0), share)


def print_worst(label, t0):
    print(f"\n  {label} ({time.time() - t0:.1f} s); worst share of the f32 allowance: " +
          ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


# ---------------------------------------------------------------------------------------------------------------- recording
class Spec:
    """geometry of one tensor argument: its storage (identity and size), dtype, shape, strides, offset"""

    def __init__(self, t, keep=False):
        self.key = t.untyped_storage().data_ptr()
        self.numel = t.untyped_storage().nbytes() // t.element_size()
        self.dtype, self.shape, self.stride, self.offset = t.dtype, tuple(t.shape), tuple(t.stride()), t.storage_offset()
        self.obj = t if keep else None          # (the RoPE tables: the replay reads the model's own)

    def view(self, buf):
        return buf.as_strided(self.shape, self.stride, self.offset)


_recordings = {}


def recording(ops, cfg, monkeypatch):
    """[(op, {argument: Spec or value})] of prepare_conditioning + denoise + prepare_modulation at configuration cfg"""
    if cfg in _recordings:
        return _recordings[cfg]
    monkeypatch.setenv("X2I_QKV_FUSE", "0")             # read at model construction
    from x2i_amd.flux import FluxTransformer2DModel
    B, side = CONFIGS[cfg]
    hw = side // 16
    Si = hw * hw
    m = FluxTransformer2DModel(num_layers=1, num_single_layers=1, guidance_embeds=True, device=DEV).init_random_(seed=3)
    assert not m.fuse_qkv
    for blk in list(m.transformer_blocks) + list(m.single_transformer_blocks):
        blk.attn.register_forward_hook(lambda mod, inp, out: None)
    g = torch.Generator().manual_seed(5)
    enc = torch.randn((B, ST, 4096), generator=g).to(DEV, torch.bfloat16)
    pooled = torch.randn((B, 768), generator=g).to(DEV, torch.bfloat16)
    img_ids = torch.zeros((hw, hw, 3))
    img_ids[..., 1] += torch.arange(hw)[:, None]
    img_ids[..., 2] += torch.arange(hw)[None, :]
    hs = torch.randn((B, Si, 64), generator=g).to(DEV, torch.bfloat16)
    calls, alive = [], []
    orig = {n: getattr(ops, n) for n in WRAPPED}
    sigs = {n: inspect.signature(f) for n, f in orig.items()}

    def wrap(n):
        def f(*a, **k):
            ba = sigs[n].bind(*a, **k)
            ba.apply_defaults()
            rec = {}
            for key, v in ba.arguments.items():
                rec[key] = Spec(v, keep=key in ("cos", "sin")) if isinstance(v, torch.Tensor) else v
            calls.append((n, rec))
            alive.extend(v for v in ba.arguments.values() if isinstance(v, torch.Tensor))   # (no storage is reused while named by address)
            return orig[n](*a, **k)
        return f
    try:
        for n in WRAPPED:
            setattr(ops, n, wrap(n))
        state = m.prepare_conditioning(enc, pooled, torch.zeros((ST, 3), device=DEV), img_ids.reshape(-1, 3).to(DEV),
                                       guidance=torch.full((B,), 3.5, device=DEV))
        m.denoise(state, hs, torch.full((B,), 0.75, device=DEV))
        n_mod = len(calls)
        steps = [torch.full((B,), t, device=DEV) for t in (1.0, 0.75, 0.5, 0.25)]
        m.prepare_modulation(state, steps, dtype=torch.bfloat16)
        torch.cuda.synchronize()
    finally:
        for n, f in orig.items():
            setattr(ops, n, f)
    rec = dict(calls=calls, B=B, Si=Si, S=ST + Si, n_denoise=n_mod, Ntot=m._mod_rows)
    del m, state, alive
    _recordings.clear()
    _recordings[cfg] = rec
    return rec


def check_launch_list(rec):
    """the launches the model is known to make, in order (x2i_amd/flux.py)"""
    B, S, Si = rec["B"], rec["S"], rec["Si"]
    names = [c[0] for c in rec["calls"]]
    sk, sn, ln, gr, qs = "skinny_linear", "timestep_sinusoid", "ln_modulate", "gated_residual_", "qkv_split"
    want = [sk, sk, sn, sk, sk,                   # text embedder, guidance: sinusoid + embedder
            sn, sk, sk, sk,                       # timestep: sinusoid + embedder, modulation table
            ln, qs, gr, gr, ln,                   # double block: norm1, split, the two gated residuals, norm2
            ln, qs,                               # single block
            ln]                                   # norm_out
    g = 4 // B
    if g >= 2:                                    # prepare_modulation: one pass of g steps per 4 // B
        want += [sn, sk, sk, sk] * ((4 + g - 1) // g)
    assert names == want, names
    calls = [c[1] for c in rec["calls"]]
    mod = calls[8]
    assert mod["W"].shape == (rec["Ntot"], D) and mod["act_in"] == E.ACT_SILU and mod["X"].shape == (B, D)
    assert calls[4]["accumulate"] and calls[7]["accumulate"]
    l1, l2, ls, lo = calls[9], calls[13], calls[14], calls[16]
    assert (l1["S"], l1["S0"], l2["S0"], ls["S0"]) == (S, ST, ST, 0)
    assert (lo["S"], lo["x_offset"], lo["x_bs"], lo["y_bs"]) == (Si, ST * D, S * D, Si * D)
    assert calls[10]["S0"] == ST and calls[15]["S0"] == 0 and calls[15]["qkv0"] is None
    assert (calls[11]["S"], calls[11]["x_offset"], calls[12]["S"]) == (Si, ST * D, ST)


# ---------------------------------------------------------------------------------------------------------------- replay
def _randn(n, gen, scale=1.0, dtype=torch.float32):
    return (scale * torch.randn(n, device=DEV, generator=gen)).to(dtype)


def _fresh(specs, fill):
    """one fresh storage per storage key, filled by fill(role, spec)"""
    bufs = {}
    for role, s in specs.items():
        if isinstance(s, Spec) and s.key not in bufs and s.obj is None:
            bufs[s.key] = fill(role, s)
    return bufs


def _mask_check(name, buf, views, old=None):
    """outside `views` the storage keeps the sentinel (old None) or its old contents"""
    mask = E.write_mask(buf, views)
    if old is None:
        E.check_untouched(name, buf, mask)
        return
    same = (buf.view(-1).view(torch.int16 if buf.element_size() == 2 else torch.int32) ==
            old.view(-1).view(torch.int16 if old.element_size() == 2 else torch.int32)) | mask
    if not bool(same.all()):
        i = int(torch.nonzero(~same)[0])
        raise AssertionError(f"{name}: {int((~same).sum())} elements outside the launch's write set changed; first at element {i}")


def replay_ln(ops, p, kind, seed, name):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    Dd = p["D"]

    def fill(role, s):
        if role == "Y":
            return E.poison_(torch.empty(s.numel, device=DEV, dtype=s.dtype))
        if role == "X":
            return E.ln_rows(s.numel // Dd, Dd, kind, gen, DEV).view(-1)
        return E.mod_vectors(s.numel, kind, gen, DEV)
    bufs = _fresh(p, fill)
    args = {k: (v.view(bufs[v.key]) if isinstance(v, Spec) else v) for k, v in p.items()}
    ops.ln_modulate(**args)
    torch.cuda.synchronize()
    B, S, S0 = p["B"], p["S"], p["S0"]
    xs, ys = p["X"], p["Y"]
    ldx = Dd if p["ldx"] is None else p["ldx"]                # (ops.ln_modulate's defaults)
    ldy = Dd if p["ldy"] is None else p["ldy"]
    x_bs = S * ldx if p["x_bs"] is None else p["x_bs"]
    y_bs = S * ldy if p["y_bs"] is None else p["y_bs"]
    X3 = bufs[xs.key].as_strided((B, S, Dd), (x_bs, ldx, 1), xs.offset + p["x_offset"])
    yv = ((B, S, Dd), (y_bs, ldy, 1), ys.offset + p["y_offset"])
    Y3 = bufs[ys.key].as_strided(*yv)

    def mv(role):
        s = p[role] if p[role] is not None else p[role[:-1] + "1"]
        return bufs[s.key].as_strided((B, Dd), (p["mod_bs"], 1), s.offset)
    rep = E.Report(f"{name} {kind}")
    E.check_ln(rep, X3, Y3, S0, mv("shift0"), mv("scale0"), mv("shift1"), mv("scale1"), p["eps"])
    share = rep.done()
    _mask_check(f"{name} {kind}", bufs[ys.key], [yv])
    return share


def replay_skinny(ops, p, kind, seed, name):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    B, K = p["X"].shape
    N = p["W"].shape[0]
    ldy = p["ldy"] if p["ldy"] is not None else (p["out"].stride[0] if p["out"] is not None else N)

    def fill(role, s):
        if role == "X":
            return _randn(s.numel, gen, 1.0, s.dtype)
        if role == "W":
            return _randn(s.numel, gen, K ** -0.5, s.dtype)
        if role == "bias":
            return _randn(s.numel, gen, 0.5, s.dtype)
        return E.poison_(torch.empty(s.numel, device=DEV, dtype=s.dtype))
    bufs = _fresh(p, fill)
    args = {k: (v.view(bufs[v.key]) if isinstance(v, Spec) else v) for k, v in p.items()}
    X, W, bias = args["X"], args["W"], args["bias"]
    if kind == "cancel" and bias is not None:        # sample 0's pre-activation is a rounding residual
        bias.copy_((-(W.double() @ E.act_f64(X[0].double(), p["act_in"]))).to(bias.dtype))
    y_old = None
    if p["out"] is not None:
        os_ = p["out"]
        yv = ((B, N), (ldy, 1), os_.offset)
        Y = bufs[os_.key].as_strided(*yv)
        if p["accumulate"]:
            Y.copy_(torch.randn((B, N), device=DEV, generator=gen))
            y_old = Y.clone()
    out = ops.skinny_linear(**args)
    torch.cuda.synchronize()
    rep = E.Report(f"{name} {kind}")
    E.check_skinny(rep, X, W, bias, out[:, :N] if p["out"] is None else Y, act_in=p["act_in"], act_out=p["act_out"], y_old=y_old)
    share = rep.done()
    if p["out"] is not None:
        _mask_check(f"{name} {kind}", bufs[os_.key], [yv])
    return share


def replay_gated(ops, p, kind, seed, name):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    Dd = p["D"]

    def fill(role, s):
        if role == "gate":
            return E.mod_vectors(s.numel, "random", gen, DEV)
        return E.ln_rows(s.numel // Dd, Dd, kind, gen, DEV).view(-1)
    bufs = _fresh(p, fill)
    args = {k: (v.view(bufs[v.key]) if isinstance(v, Spec) else v) for k, v in p.items()}
    B, S = p["B"], p["S"]
    xs, ts, gs = p["X"], p["T"], p["gate"]
    xv = ((B, S, Dd), (p["x_bs"], p["ldx"], 1), xs.offset + p["x_offset"])
    X3 = bufs[xs.key].as_strided(*xv)
    T3 = bufs[ts.key].as_strided((B, S, Dd), (p["t_bs"], p["ldt"], 1), ts.offset + p["t_offset"])
    G = bufs[gs.key].as_strided((B, Dd), (p["gate_bs"], 1), gs.offset)
    old = bufs[xs.key].clone()
    X_old = X3.clone()
    ops.gated_residual_(**args)
    torch.cuda.synchronize()
    rep = E.Report(f"{name} {kind}")
    E.check_gated(rep, X_old, T3, G, X3)
    share = rep.done()
    _mask_check(f"{name} {kind}", bufs[xs.key], [xv], old=old)
    return share


def replay_qkv_split(ops, p, kind, seed, name):
    gen = torch.Generator(device=DEV).manual_seed(seed)

    def fill(role, s):
        if role in ("Q", "K", "VT"):
            return E.poison_(torch.empty(s.numel, device=DEV, dtype=s.dtype))
        if role.startswith("n"):
            return (1.0 + 0.1 * torch.randn(s.numel, device=DEV, generator=gen)).to(s.dtype)
        return E.ln_rows(s.numel // 128, 128, kind, gen, DEV).view(-1)
    bufs = _fresh(p, fill)
    args = {k: (v.obj if isinstance(v, Spec) and v.obj is not None else v.view(bufs[v.key]) if isinstance(v, Spec) else v)
            for k, v in p.items()}
    ops.qkv_split(**args)
    torch.cuda.synchronize()
    B, S, S0, H = p["B"], p["S"], p["S0"], p["H"]
    rows = E.qkv_split_rows_of(args["qkv0"], args["qkv1"], p["ld0"], p["ld1"], B, S, S0, H)
    rep = E.Report(f"{name} {kind}")
    E.check_qkv_split(rep, rows, args["nq0"], args["nk0"], args["nq1"], args["nk1"], args["cos"], args["sin"], args["Q"], args["K"],
                      args["VT"], S=S, S0=S0, H=H, eps=p["eps"])
    share = rep.done()
    E.check_qkv_split_padding(f"{name} {kind}", args["Q"], args["K"], args["VT"], S)
    for r in ("Q", "K", "VT"):           # whole storages: nothing outside the views
        s = p[r]
        _mask_check(f"{name} {kind} {r}", bufs[s.key], [(s.shape, s.stride, s.offset)])
    return share


def sinusoid_t(n, kind, gen):
    if kind == "random":
        return 1000.0 * torch.rand(n, device=DEV, generator=gen)
    if kind == "bf16_grid":      # what the model passes: (t.bf16() * 1000) in bf16, then f32
        return ((torch.rand(n, device=DEV, generator=gen).to(torch.bfloat16) * 1000)).float()
    edge = torch.tensor([0.0, 1000.0, 3500.0, 1e-3, 999.0, 752.0, 0.5, 4000.0], device=DEV)
    return edge[torch.arange(n, device=DEV) % 8]


def replay_sinusoid(ops, p, kind, seed, name):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    t = sinusoid_t(p["t"].shape[0], kind, gen)
    out = ops.timestep_sinusoid(t, p["dim"], round_bf16=p["round_bf16"])
    torch.cuda.synchronize()
    return sinusoid_check(f"{name} {kind}", t, out, p["dim"], p["round_bf16"])


def sinusoid_check(name, t, out, dim, round_bf16):
    want, bound, delta = E.sinusoid_expect(t, dim, round_bf16)
    if round_bf16:       # the value is a bf16 one, stored as f32
        assert torch.equal(out, out.to(torch.bfloat16).float()), name
    rep = E.Report(name)
    rep.check(out, want, bound, delta, sample=torch.arange(t.shape[0], device=DEV), token=torch.zeros(t.shape[0], dtype=torch.long, device=DEV),
              unit=1)
    return rep.done()


REPLAY = {"ln_modulate": replay_ln, "skinny_linear": replay_skinny, "gated_residual_": replay_gated, "qkv_split": replay_qkv_split,
          "timestep_sinusoid": replay_sinusoid}


def launch_name(rec, i):
    op, p = rec["calls"][i]
    tags = {0: "text_emb.1", 1: "text_emb.2", 2: "guid_sin", 3: "guid_emb.1", 4: "guid_emb.2", 5: "time_sin", 6: "time_emb.1",
            7: "time_emb.2", 8: "mod_table", 9: "ln_norm1", 10: "qkv_split_double", 11: "gated_img", 12: "gated_txt", 13: "ln_norm2",
            14: "ln_single", 15: "qkv_split_single", 16: "ln_norm_out"}
    if i in tags:
        return tags[i]
    return "prep_mod_" + {"timestep_sinusoid": "sin", "skinny_linear": "skinny"}[op] + f"#{i}"


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_model_elementwise_launches_vs_fp64(ops, cfg, monkeypatch):
    t0 = time.time()
    rec = recording(ops, cfg, monkeypatch)
    check_launch_list(rec)
    n = 0
    for i, (op, p) in enumerate(rec["calls"]):
        name = launch_name(rec, i)
        for j, kind in enumerate(KINDS[op]):
            share = REPLAY[op](ops, p, kind, 1000 * i + j, f"{cfg} {name}")
            note(name if not name.startswith("prep_mod") else "prep_mod_" + op, share)
            n += 1
    print(f"\n  {cfg}: {len(rec['calls'])} launches, {n} replays")
    print_worst(cfg, t0)


# ---------------------------------------------------------------------------------------------------------------- unit launches: skinny
def _skinny_unit(ops, X, W, bias, *, N, ldy, act_in=E.ACT_NONE, act_out=E.ACT_NONE, accumulate=False, y_old=None, name, rows=65536):
    B = X.shape[0]
    buf = E.poison_(torch.empty(B * ldy + 7, device=DEV))
    Y = buf[:B * ldy].view(B, ldy)[:, :N]
    if accumulate:
        Y.copy_(y_old)
    ops.skinny_linear(X, W, bias, out=Y, act_in=act_in, act_out=act_out, accumulate=accumulate, ldy=ldy)
    torch.cuda.synchronize()
    rep = E.Report(name)
    E.check_skinny(rep, X, W, bias, Y, act_in=act_in, act_out=act_out, y_old=y_old if accumulate else None, rows=rows)
    share = rep.done()
    E.check_untouched(name, buf, E.write_mask(buf, [((B, N), (ldy, 1), 0)]), row_len=ldy)
    return Y.clone(), share


def _rand_w(N, K, gen, chunk=65536):
    W = torch.empty((N, K), device=DEV, dtype=torch.bfloat16)
    for n0 in range(0, N, chunk):
        n1 = min(N, n0 + chunk)
        W[n0:n1] = (K ** -0.5 * torch.randn((n1 - n0, K), device=DEV, generator=gen)).to(torch.bfloat16)
    return W


def test_skinny_full_depth_modulation_table(ops):
    """the full-depth AdaLN table: N = 344 D (19 double + 38 single blocks + norm_out), K = D, SiLU in, rpw = 16, at B = 1, 2 and 4; each
    sample's row bit-identical to its own single-sample launch"""
    t0 = time.time()
    gen = torch.Generator(device=DEV).manual_seed(21)
    N, K = 344 * D, D
    W = _rand_w(N, K, gen)
    bias = (0.5 * torch.randn(N, device=DEV, generator=gen)).to(torch.bfloat16)
    X = 2.0 * torch.randn((4, K), device=DEV, generator=gen)
    single = [ops.skinny_linear(X[b:b + 1].contiguous(), W, bias, act_in=E.ACT_SILU) for b in range(4)]
    for B in (1, 2, 4):
        Y, share = _skinny_unit(ops, X[:B].contiguous(), W, bias, N=N, ldy=N, act_in=E.ACT_SILU, name=f"mod_table_full B={B}")
        note("unit_mod_table_full", share)
        for b in range(B):
            assert torch.equal(Y[b], single[b][0]), (B, b)
    # cancel: sample 0's pre-activation is the rounding residual of -bias
    bias_c = torch.empty_like(bias)
    for n0 in range(0, N, 65536):
        bias_c[n0:n0 + 65536] = (-(W[n0:n0 + 65536].double() @ E.act_f64(X[0].double(), E.ACT_SILU))).to(torch.bfloat16)
    _, share = _skinny_unit(ops, X[:2].contiguous(), W, bias_c, N=N, ldy=N, act_in=E.ACT_SILU, name="mod_table_full cancel")
    note("unit_mod_table_full", share)
    del W
    print_worst("full-depth modulation table", t0)


@pytest.mark.parametrize("N", [65536 + 43, 65536 - 13], ids=["rpw16", "rpw4"])
def test_skinny_ragged_n_around_rpw_switch(ops, N):
    t0 = time.time()
    gen = torch.Generator(device=DEV).manual_seed(N)
    K = D
    W = _rand_w(N, K, gen)
    bias = (0.5 * torch.randn(N, device=DEV, generator=gen)).to(torch.bfloat16)
    X = torch.randn((3, K), device=DEV, generator=gen)
    y_old = torch.randn((3, N), device=DEV, generator=gen)
    for acc in (False, True):
        _, share = _skinny_unit(ops, X, W, bias, N=N, ldy=N + 20, act_in=E.ACT_SILU, accumulate=acc, y_old=y_old,
                                name=f"skinny N={N} acc={acc}")
        note(f"unit_skinny_N{N}", share)
    print_worst(f"skinny N = {N}", t0)


@pytest.mark.parametrize("K", [256, 768, 3072])
@pytest.mark.parametrize("accumulate", [False, True], ids=["plain", "accumulate"])
def test_skinny_batch_sweep(ops, K, accumulate):
    """B = 1 .. 9, 13, 16 (B > 8: several launches of up to 8 rows), ragged N = 1000, ldy > N; f32 input with SiLU in and bf16 input with
    SiLU out; every sample's row bit-identical to the B = 16 launch's"""
    t0 = time.time()
    gen = torch.Generator(device=DEV).manual_seed(K + accumulate)
    N, ldy = 1000, 1000 + 24
    W = _rand_w(N, K, gen)
    bias = (0.5 * torch.randn(N, device=DEV, generator=gen)).to(torch.bfloat16)
    X = torch.randn((16, K), device=DEV, generator=gen)
    y_old = torch.randn((16, N), device=DEV, generator=gen)
    for xin, a_in, a_out in ((X, E.ACT_SILU, E.ACT_NONE), (X.to(torch.bfloat16), E.ACT_NONE, E.ACT_SILU)):
        full, _ = _skinny_unit(ops, xin, W, bias, N=N, ldy=ldy, act_in=a_in, act_out=a_out, accumulate=accumulate, y_old=y_old,
                               name=f"skinny K={K} B=16")
        for B in list(range(1, 10)) + [13, 16]:
            Y, share = _skinny_unit(ops, xin[:B].contiguous(), W, bias, N=N, ldy=ldy, act_in=a_in, act_out=a_out, accumulate=accumulate,
                                    y_old=y_old[:B], name=f"skinny K={K} B={B} {xin.dtype} acc={accumulate}")
            note(f"unit_skinny_K{K}", share)
            bad = [b for b in range(B) if not torch.equal(Y[b], full[b])]
            assert not bad, f"K={K} B={B}: samples {bad} differ from the B = 16 launch"
    print_worst(f"skinny K = {K}", t0)


# ---------------------------------------------------------------------------------------------------------------- unit launches: LN, Euler, sinusoid
LN_UNITS = [  # (B, S, S0, D, padded strides): B S >= 4096 at D = 3072 -> ln_rows_kernel; 4113 rows: not a multiple of 16
    (3, 1371, 117, 3072, True), (3, 1371, 117, 3072, False), (1, 4113, 0, 3072, True), (5, 821, 3, 3072, True),
    (2, 1001, 513, 3072, True),                                          # 2002 rows: ln_kernel
    (3, 37, 13, 1024, True), (2, 50, 18, 4096, False)]                   # other widths: ln_kernel


@pytest.mark.parametrize("B,S,S0,Dd,pad", LN_UNITS)
def test_ln_unit_launches(ops, B, S, S0, Dd, pad):
    t0 = time.time()
    ldx, ldy = (Dd + 32, Dd + 64) if pad else (Dd, Dd)
    x_bs, y_bs = (S * ldx + 64, S * ldy + 128) if pad else (S * ldx, S * ldy)
    x_off, y_off = (8, 16) if pad else (0, 0)
    mod_bs = 4 * Dd + (12 if pad else 0)
    for j, kind in enumerate(E.LN_KINDS):
        gen = torch.Generator(device=DEV).manual_seed(100 * j + S)
        xbuf = E.ln_rows((B * x_bs + x_off + Dd) // Dd + 1, Dd, "random", gen, DEV).view(-1)
        X3 = xbuf.as_strided((B, S, Dd), (x_bs, ldx, 1), x_off)
        X3.copy_(E.ln_rows(B * S, Dd, kind, gen, DEV).view(B, S, Dd))
        ybuf = E.poison_(torch.empty(B * y_bs + y_off + 64, device=DEV, dtype=torch.bfloat16))
        mbuf = E.mod_vectors(B * mod_bs, kind, gen, DEV)
        MOD = mbuf.view(B, mod_bs)
        sh0, sc0, sh1, sc1 = (MOD[:, i * Dd:] for i in range(4))
        ops.ln_modulate(xbuf, ybuf, B, S, Dd, S0, sh0 if S0 else None, sc0 if S0 else None, sh1, sc1, mod_bs, x_bs=x_bs, ldx=ldx,
                        y_bs=y_bs, ldy=ldy, x_offset=x_off, y_offset=y_off)
        torch.cuda.synchronize()
        yv = ((B, S, Dd), (y_bs, ldy, 1), y_off)
        name = f"ln B={B} S={S} S0={S0} D={Dd} pad={pad} {kind}"
        rep = E.check_ln(E.Report(name), X3, ybuf.as_strided(*yv), S0, sh0 if S0 else sh1, sc0 if S0 else sc1, sh1, sc1, 1e-6)
        note(f"unit_ln_D{Dd}", rep.done())
        E.check_untouched(name, ybuf, E.write_mask(ybuf, [yv]), row_len=ldy)
    print_worst(f"ln B={B} S={S} S0={S0} D={Dd}", t0)


@pytest.mark.parametrize("n,off", [(2 * 4096 * 64, 0), (2 * 4096 * 64 - 3, 0), (4 * 1021 * 64 + 5, 1), (13, 0)],
                         ids=["model", "tail", "misaligned", "short"])
def test_euler_step_vs_fp64(ops, n, off):
    """euler_step_ on the latent of 1024^2 (vector kernel), n % 8 != 0 (vector kernel + euler_tail_kernel), a view 2 bytes off 16-byte
    alignment (euler_tail_kernel only): within one rounding of x + dt e, nothing outside x written"""
    gen = torch.Generator(device=DEV).manual_seed(n)
    xbuf = torch.randn(n + off + 16, device=DEV, generator=gen).to(torch.bfloat16)
    e = torch.randn(n, device=DEV, generator=gen).to(torch.bfloat16)
    old = xbuf.clone()
    x = xbuf[off:off + n]
    dt = torch.tensor([-0.0625 * 3.3], device=DEV)
    ops.euler_step_(x, e, dt)
    torch.cuda.synchronize()
    want, bound, delta = E.euler_expect(old[off:off + n], e, float(dt))
    i = torch.arange(n, device=DEV)
    rep = E.Report(f"euler n={n} off={off}")
    rep.check(x[:, None], want[:, None], bound[:, None], delta[:, None], sample=i * 0, token=i, unit=1)
    note("unit_euler", rep.done())
    assert torch.equal(xbuf[:off], old[:off]) and torch.equal(xbuf[off + n:], old[off + n:])


@pytest.mark.parametrize("dim", [256, 128])
@pytest.mark.parametrize("round_bf16", [False, True])
def test_sinusoid_sweep(ops, dim, round_bf16):
    """t over [0, 1000] in steps of 1/8 (the sampler's t 1000 values), the bf16 grid of t 1000, guidance scales 1 .. 10 x 1000"""
    t = torch.cat((torch.arange(0, 8001, device=DEV) / 8.0, (torch.linspace(0, 1, 1001, device=DEV).to(torch.bfloat16) * 1000).float(),
                   torch.linspace(1000, 10000, 37, device=DEV)))
    out = ops.timestep_sinusoid(t.contiguous(), dim, round_bf16=round_bf16)
    torch.cuda.synchronize()
    note("unit_sinusoid", sinusoid_check(f"sinusoid dim={dim} round={round_bf16}", t, out, dim, round_bf16))


def test_print_worst():
    """(last: the table of worst shares over everything this module ran)"""
    print_worst("all", time.time())
