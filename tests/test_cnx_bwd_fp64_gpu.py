"""Every ControlNeXt backward launch (csrc/conv_bwd.hip, the batched GEMMs of lightcontrol_train.dgrad_2x2s2) against the float64 references
of tests/cnx_bwd_ref.py -- every output element, NaN fails, every written buffer starts as the sentinel (or as a saved copy where the launch
accumulates or works in place), and everything outside a launch's write set is checked unchanged: dw, db and dpre when they are not asked
for, and a margin behind dx.

(a) x2i_groupnorm_nhwc_bwd_bf16 unit launches.  Shapes (B, HW, C, G) and what each reaches:
      (2, 560, 64, 2), (2, 560, 128, 4), (2, 560, 256, 8)   the trainer tests' geometry: chunk 63 is no multiple of the 32 / 16 / 8 rows per
                                                             block and the last chunk is short
      (1, 1, 8, 1)                                           HW = 1, C = 8, G = 1: 256 rows per block of which one is live
      (3, 63, 8, 8), (3, 64, 8, 2), (3, 65, 8, 1)            one chunk and the first split into two; one channel per group
      (1, 130, 512, 32)                                      4 rows per block
      (2, 70, 1024, 512), (2, 70, 1024, 1024)                2 rows per block, the g += 256 loops, one channel per group
      (1, 7300, 64, 2)                                       115 chunks: reduce_rows' 8-deep loop
      (5, 300, 128, 8)                                       odd B, the sample loop of dw
    Options per shape: cnx_bwd_ref.gn_bwd_cases (in_relu; pre_add + dpre; dx_in separate and aliased by dx; dw / db None, plain, accumulated;
    the activations rotating; the trainer's eight combinations).  Operands: every conv_ref.GN_KINDS kind for x / pre_add, dy ~ N(0, 1) and
    `tagged` alternating.
(b) x2i_linear_wgrad_f32: (1, 1, 1) one thread of each sort; (3, 24, 16) N K + N = 408, the bias threads straddle a block edge;
    (8, 128, 256) N K a multiple of 256, the bias threads alone in the last block; (9, 40, 50) B past the skinny kernels' 8; the trainer's four.
(c) x2i_conv_stem_wgrad_bf16: (1, 8, 8, 64) one block of 16 pixels; (3, 50, 36, 64) the old test's case; (2, 51, 37, 64) odd H and W;
    (2, 51, 37, 32) idle lanes; (1, 128, 130, 64) several blocks with a ragged last one.
(d) One recorded ControlNeXtTrainer backward (one net, 128 x 128 hint, B = 2, the output gradient inside a wider token buffer): the launch
    list asserted in order, every launch replayed at its recorded geometry on fresh poisoned storage.  Read off _backward_net the list
    holds 12 conv weight gradients, 2 B GEMMs, 9 GroupNorm backwards, 1 stem and 4 linear weight gradients.
(e) Negative controls on real kernel output.

WORST keeps the largest share of the allowance per kernel, output and operand kind; test_print_worst prints the tables."""
import time

import pytest
import torch

from tests import cnx_bwd_ref as R
from tests import gemm_ref as GREF
from tests import gemm_replay as GR
from tests.conv_ref import GN_KINDS
from tests.gemm_ref import ACT_NONE, ACT_RELU, ACT_SILU, check_untouched, poison_, write_mask

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}      # (kernel, output, operand kind) -> worst share of the allowance
STAT = {}       # operand kind -> largest median share of the statistics' allowance in half an output ulp (groupnorm_bwd dx)
REACHED = {}    # rows per block -> set of what ran there
MARGIN = 4096
# last_gemm_tile of the 2 B GEMMs of dgrad_2x2s2 in the recorded step (M = 8 rows x 8 items, N = 512, K = 3072), measured on MI355X
GEMM_FORM = 128
FORMS_SEEN = {}


@pytest.fixture(scope="module")
def ops():
    from x2i_amd import ops as o
    o._lib.load()
    return o


def note(kernel, kind, shares):
    for out, v in shares.items():
        WORST[(kernel, out, kind)] = max(WORST.get((kernel, out, kind), 0.0), v)


def pool(sizes, prev=None, skip=()):
    """one poisoned f32 storage holding the named pieces back to back and a margin; prev {name: tensor}: the contents before an accumulating
    launch (the pieces in `skip`, which the launch is not given, stay the sentinel).  Returns (storage, {name: view}, {name: (offset, size)})"""
    buf = poison_(torch.empty(sum(sizes.values()) + 64, device=DEV, dtype=torch.float32))
    views, where, off = {}, {}, 0
    for k, n in sizes.items():
        views[k], where[k] = buf[off:off + n], (off, n)
        if prev and prev.get(k) is not None and k not in skip:
            views[k].copy_(prev[k].reshape(-1))
        off += n
    return buf, views, where


def pool_untouched(name, buf, where, written):
    check_untouched(name, buf, write_mask(buf, [((where[k][1],), (1,), where[k][0]) for k in written]))


# ---------------------------------------------------------------------------------------------------------------- (a) GroupNorm backward
def run_gn(ops, c, kind, dyk, seed, name, expect_case=None):
    (B, HW, C, G) = c["shape"]
    o = R.gn_bwd_operands(c, kind, dyk, seed, DEV)
    n = B * HW * C
    dxbuf = poison_(torch.empty(n + MARGIN, device=DEV, dtype=torch.bfloat16))
    dx = dxbuf[:n].view(B, HW, C)
    dx_in = o["dx_in"]
    if c["dx_in"] == "alias":
        dx.copy_(o["dx_in"])
        dx_in = dx
    acc = c["dw"] == "acc"
    fbuf, v, where = pool(dict(dw=C, db=C, dpre=B * C), dict(dw=o["prev_dw"], db=o["prev_db"]) if acc else None)
    with_dw, with_dpre = c["dw"] != "none", o["pre_add"] is not None
    ops.groupnorm_bwd(o["x"], o["dy"], o["w"], o["b"], G, c["eps"], act=c["act"], pre_add=o["pre_add"], dpre=v["dpre"].view(B, C) if with_dpre else None,
                      dx_in=dx_in, dx=dx, dw=v["dw"] if with_dw else None, db=v["db"] if with_dw else None, in_relu=c["in_relu"], accumulate=acc)
    torch.cuda.synchronize()
    exp = R.gn_bwd_expect_case(expect_case or c, o)
    shares = R.check_gn_bwd(name, exp, dx, G, dx_in=o["dx_in"], dw=v["dw"] if with_dw else None, db=v["db"] if with_dw else None,
                            dpre=v["dpre"].view(B, C) if with_dpre else None)
    check_untouched(name + " (behind dx)", dxbuf, write_mask(dxbuf, [((n,), (1,), 0)]))
    pool_untouched(name + " (dw / db / dpre not asked for)", fbuf, where, (["dw", "db"] if with_dw else []) + (["dpre"] if with_dpre else []))
    note("groupnorm_bwd", kind, shares)
    STAT[kind] = max(STAT.get(kind, 0.0), exp["stat_share"])
    pl = R.gn_bwd_plan(B, HW, C, G)
    REACHED.setdefault(pl["rows"], set()).update(
        [kind, "dy " + dyk, R.ACT_NAME[c["act"]], "dx_in " + c["dx_in"], "dw " + c["dw"]] + (["in_relu"] if c["in_relu"] else []) +
        (["pre_add+dpre"] if with_dpre else []) + (["G>256"] if G > 256 else []) + (["one chunk"] if pl["nchunk"] == 1 else []) +
        ([">112 chunks"] if pl["nchunk"] > 112 else []) + (["cg=1"] if C == G else []) + (["odd B"] if B % 2 else []))
    return shares, exp


GN_CASES = R.gn_bwd_cases()


@pytest.mark.parametrize("i", range(len(GN_CASES)), ids=[R.case_id(c) for c in GN_CASES])
def test_groupnorm_bwd_unit_launches_vs_fp64(ops, i):
    c, t0, out = GN_CASES[i], time.time(), []
    for k, kind in enumerate(GN_KINDS):
        shares, exp = run_gn(ops, c, kind, "tagged" if (i + k) % 2 else "random", 100 + 7 * i + k, f"{R.case_id(c)} {kind}")
        out.append(f"{kind} " + "/".join(f"{o} {v:.3f}" for o, v in shares.items()) + f" stat {exp['stat_share']:.2g} und {exp['undecided']}")
    print(f"\n  {R.case_id(c)} ({time.time() - t0:.1f} s): " + "; ".join(out))


def test_groupnorm_bwd_relaunch_is_bit_identical(ops):
    c = GN_CASES[1]
    o = R.gn_bwd_operands(c, "random", "random", 5, DEV)
    B, HW, C, G = c["shape"]
    outs = []
    for _ in range(2):
        dw, db, dpre = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), torch.empty((B, C), device=DEV)
        dx = ops.groupnorm_bwd(o["x"], o["dy"], o["w"], o["b"], G, c["eps"], act=c["act"], pre_add=o["pre_add"], dpre=dpre, dx_in=o["dx_in"], dw=dw, db=db)
        outs.append((dx, dw, db, dpre))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(*outs))


# ---------------------------------------------------------------------------------------------------------------- (b) linear_wgrad
TRAINER_LINEAR = [(2, 128, 256, ACT_SILU), (2, 256, 256, ACT_SILU), (2, 256, 256, ACT_NONE), (2, 256, 128, ACT_NONE)]
LINEAR_SHAPES = [(1, 1, 1), (3, 24, 16), (8, 128, 256), (9, 40, 50)] + sorted({s[:3] for s in TRAINER_LINEAR})


def run_linear(ops, B, N, K, act, with_db, acc, seed, name):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s: torch.randn(s, device=DEV, generator=gen)
    dy, x = rn(B, N), 3.0 * rn(B, K)
    prev = dict(dw=rn(N, K), db=rn(N)) if acc else None
    fbuf, v, where = pool(dict(dw=N * K, db=N), prev, () if with_db else ("db",))
    ops.linear_wgrad(dy, x, v["dw"].view(N, K), v["db"] if with_db else None, act_in=act, accumulate=acc)
    torch.cuda.synchronize()
    (ww, wb_), (bw, bb) = R.linear_wgrad_expect(dy, x, act, prev["dw"] if acc else None, prev["db"] if acc else None)
    shares = dict(dw=R.check_vec(name + " dw", v["dw"], ww, wb_, R.where_linear(K)))
    if with_db:
        shares["db"] = R.check_vec(name + " db", v["db"], bw, bb, lambda i: f"db[n={i}]")
    pool_untouched(name, fbuf, where, ["dw"] + (["db"] if with_db else []))
    note("linear_wgrad", R.ACT_NAME[act], shares)
    return shares


@pytest.mark.parametrize("B,N,K", LINEAR_SHAPES)
def test_linear_wgrad_vs_fp64(ops, B, N, K):
    out = []
    for act in (ACT_NONE, ACT_SILU):
        for with_db in (True, False):
            for acc in (False, True):
                sh = run_linear(ops, B, N, K, act, with_db, acc, 3 + B + N + K, f"linear_wgrad {B, N, K} {R.ACT_NAME[act]} db={with_db} acc={acc}")
                out.append(max(sh.values()))
    print(f"\n  linear_wgrad {B, N, K}: worst share {max(out):.3f}")


# ---------------------------------------------------------------------------------------------------------------- (c) conv_stem_wgrad
STEM_SHAPES = [(1, 8, 8, 64), (3, 50, 36, 64), (2, 51, 37, 64), (2, 51, 37, 32), (1, 128, 130, 64)]


def run_stem(ops, B, H, W, Cout, kind, with_db, acc, seed, name):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x, dy = R.wgrad_operands(kind, B, H, W, 3, (H + 1) // 2, (W + 1) // 2, Cout, 3, 3, gen, DEV)
    rn = lambda *s: torch.randn(s, device=DEV, generator=gen)
    prev = dict(dw=rn(Cout * 27), db=rn(Cout)) if acc else None
    fbuf, v, where = pool(dict(dw=Cout * 27, db=Cout), prev, () if with_db else ("db",))
    ops.conv_stem_wgrad(x, dy, v["dw"], v["db"] if with_db else None, accumulate=acc)
    torch.cuda.synchronize()
    (ww, wb_), (bw, bb) = R.stem_wgrad_expect(x, dy, prev["dw"].view(Cout, 3, 3, 3) if acc else None, prev["db"] if acc else None)
    shares = dict(dw=R.check_vec(name + " dw", v["dw"], ww, wb_, R.where_wgrad(3, 3, 3)))
    if with_db:
        shares["db"] = R.check_vec(name + " db", v["db"], bw, bb, lambda i: f"db[co={i}]")
    pool_untouched(name, fbuf, where, ["dw"] + (["db"] if with_db else []))
    note("conv_stem_wgrad", kind, shares)
    return shares


@pytest.mark.parametrize("B,H,W,Cout", STEM_SHAPES)
def test_conv_stem_wgrad_vs_fp64(ops, B, H, W, Cout):
    out = []
    for kind in ("random", "tagged"):
        for with_db in (True, False):
            for acc in (False, True):
                sh = run_stem(ops, B, H, W, Cout, kind, with_db, acc, 9 + H + W, f"conv_stem_wgrad {B, H, W, Cout} {kind} db={with_db} acc={acc}")
                out.append(max(sh.values()))
    pl = R.stem_plan(B, H, W, Cout)
    print(f"\n  conv_stem_wgrad {B, H, W, Cout}: {pl['nblk']} blocks of {pl['chunk']} pixels, depth {pl['depth']}; worst share {max(out):.3f}")


# ---------------------------------------------------------------------------------------------------------------- (d) a recorded step
W_, N_, M_, S_, L_ = "conv_wgrad", "groupnorm_bwd", "gemm", "conv_stem_wgrad", "linear_wgrad"
BATCH = 2
# _backward_net in order: mid_convs.1 and its data gradient; mid_convs.0; down_sample.1; down_res.1; down_sample.0; down_res.0; embedding; time
EXPECTED = ([W_] + [M_] * (2 * BATCH) + [N_, W_, N_, W_] + [W_] + [W_, W_, N_, W_, N_] + [W_] + [W_, N_, W_, N_] + [N_, W_, N_, W_, N_, S_] +
            [L_] * 4)
_rec = {}


def _ptr(t):
    return None if t is None else t.data_ptr()


def recording(ops):
    """[(op, record)] of one ControlNeXtTrainer.backward: the net and the hint as test_conv_fp64_gpu.recording(ops, "controlnext_train")
    builds them; the output gradient sits inside a wider token buffer (offset, batch stride, row stride), as the LightControl step hands it over"""
    if _rec:
        return _rec["calls"]
    from oracle import flux as OF
    from x2i_amd.lightcontrol import ControlNeXtModel
    from x2i_amd.lightcontrol_train import ControlNeXtTrainer
    g = torch.Generator().manual_seed(7)
    m = ControlNeXtModel(device=DEV)
    m.load_state_dict({k: v.to(torch.bfloat16) for k, v in OF.random_controlnext_state_dict(seed=3).items()}, strict=True)
    hint = torch.rand((BATCH, 3, 128, 128), generator=g).to(DEV, torch.bfloat16)
    tr = ControlNeXtTrainer([m])
    out = tr.forward(hint, torch.full((BATCH,), 750.0, device=DEV))[0]
    _, ho, wo, co = out.shape
    St, ld = 5, co + 64
    S = ho * wo + St
    buf = torch.zeros((BATCH, S, ld), device=DEV, dtype=torch.bfloat16)
    buf[:, St:, :co] = torch.randn((BATCH, ho * wo, co), device=DEV).to(torch.bfloat16)
    calls, alive = [], []

    def rec_gn(x, dy, weight, bias, G, eps, act=ACT_NONE, pre_add=None, dpre=None, dx_in=None, dx=None, dw=None, db=None, in_relu=False, accumulate=False):
        B, C = x.shape[0], x.shape[-1]
        alias = dx is not None and dx_in is not None and _ptr(dx) == _ptr(dx_in)
        return dict(shape=(B, x.numel() // (B * C), C, G), act=act, eps=eps, in_relu=bool(in_relu), pre=pre_add is not None, dpre=dpre is not None,
                    dx_in="none" if dx_in is None else ("alias" if alias else "sep"), dw="none" if dw is None else ("acc" if accumulate else "plain"))

    def rec_wgrad(x, dy, dw, db, H, W, Cin, OH, OW, Cout, KH, KW, stride, pad, *, B=None, dy_offset=0, dy_batch_stride=None, ldy=None, accumulate=False):
        return dict(B=x.shape[0] if B is None else B, H=H, W=W, Cin=Cin, OH=OH, OW=OW, Cout=Cout, KH=KH, KW=KW, stride=stride, pad=pad,
                    dy_offset=dy_offset, dy_batch_stride=OH * OW * (ldy or Cout) if dy_batch_stride is None else dy_batch_stride, ldy=ldy or Cout,
                    dy_numel=dy.numel(), accumulate=bool(accumulate), db=db is not None)

    def rec_stem(x, dy, dw, db, accumulate=False):
        return dict(B=x.shape[0], H=x.shape[1], W=x.shape[2], Cout=dy.shape[-1], accumulate=bool(accumulate), db=db is not None)

    def rec_linear(dy, x, dw, db, act_in=ACT_NONE, accumulate=False):
        return dict(B=dy.shape[0], N=dy.shape[1], K=x.shape[1], act_in=act_in, accumulate=bool(accumulate), db=db is not None)

    def rec_gemm(*a, **k):
        return GR._record(dict(zip(("A", "W", "bias", "out"), a), **k))
    recs = {N_: rec_gn, W_: rec_wgrad, S_: rec_stem, L_: rec_linear, M_: rec_gemm}
    orig = {n: getattr(ops, n) for n in recs}

    def wrap(n):
        def f(*a, **k):
            calls.append((n, recs[n](*a, **k)))
            alive.extend(list(a) + list(k.values()))
            ret = orig[n](*a, **k)
            alive.append(ret)
            return ret
        return f
    try:
        for n in recs:
            setattr(ops, n, wrap(n))
        tr.backward([buf], offset=St * ld, batch_stride=S * ld, ld=ld)
        torch.cuda.synchronize()
    finally:
        for n, f in orig.items():
            setattr(ops, n, f)
    del alive
    _rec["calls"] = calls
    return calls


def test_recorded_step_launch_list(ops):
    calls = recording(ops)
    names = [c[0] for c in calls]
    assert names == EXPECTED, names
    assert (names.count(N_), names.count(W_), names.count(S_), names.count(L_), names.count(M_)) == (9, 12, 1, 4, 2 * BATCH)
    lin = [(r["B"], r["N"], r["K"], r["act_in"]) for n, r in calls if n == L_]
    assert lin == TRAINER_LINEAR, lin
    gn = [(r["shape"][2], r["shape"][3], r["eps"], r["act"], r["pre"], r["in_relu"]) for n, r in calls if n == N_]
    assert set(gn) == set(R.TRAINER_GN_CASES), gn
    assert [r["dx_in"] for n, r in calls if n == N_].count("alias") == 1                    # down_res.1.norm1
    first = calls[0][1]                                                                       # mid_convs.1: dy inside the token buffer
    assert first["dy_offset"] > 0 and first["ldy"] == first["Cout"] + 64 and first["dy_batch_stride"] > first["OH"] * first["OW"] * first["ldy"]
    for n, r in calls:
        if n == M_:
            assert r["a_offset"] >= first["dy_offset"] and r["lda"] == first["ldy"] and r["ldc"] == 512 and r["M"] == 8 and r["batch"] == 8, \
                {k: v for k, v in r.items() if not isinstance(v, GR.Spec)}
    print("\n  " + " ".join(names))


def replay_wgrad(ops, r, kind, seed, name):
    B, H, W, Cin, OH, OW, Cout, KH, KW = (r[k] for k in ("B", "H", "W", "Cin", "OH", "OW", "Cout", "KH", "KW"))
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x, dy = R.wgrad_operands(kind, B, H, W, Cin, OH, OW, Cout, KH, KW, gen, DEV)
    store = torch.full((r["dy_numel"],), float("nan"), device=DEV, dtype=torch.bfloat16)      # (a read outside the view turns the sums NaN)
    store.as_strided((B, OH * OW, Cout), (r["dy_batch_stride"], r["ldy"], 1), r["dy_offset"]).copy_(dy.view(B, OH * OW, Cout))
    rn = lambda *s: torch.randn(s, device=DEV, generator=gen)
    n = Cout * Cin * KH * KW
    prev = dict(dw=rn(n), db=rn(Cout)) if r["accumulate"] else None
    fbuf, v, where = pool(dict(dw=n, db=Cout), prev, () if r["db"] else ("db",))
    ops.conv_wgrad(x, store, v["dw"], v["db"] if r["db"] else None, H, W, Cin, OH, OW, Cout, KH, KW, r["stride"], r["pad"], B=B,
                   dy_offset=r["dy_offset"], dy_batch_stride=r["dy_batch_stride"], ldy=r["ldy"], accumulate=r["accumulate"])
    torch.cuda.synchronize()
    steps, nsplit = R._wgrad_bound_terms(B, OH, OW, Cin, Cout, KH)
    (ww, wb_), (bw, bb) = R.conv_wgrad_expect(x, dy, KH, KW, r["stride"], r["pad"], steps, nsplit,
                                              prev["dw"].view(Cout, Cin, KH, KW) if prev else None, prev["db"] if prev else None)
    shares = dict(dw=R.check_vec(name + " dw", v["dw"], ww, wb_, R.where_wgrad(Cin, KH, KW)))
    if r["db"]:
        shares["db"] = R.check_vec(name + " db", v["db"], bw, bb, lambda i: f"db[co={i}]")
    pool_untouched(name, fbuf, where, ["dw"] + (["db"] if r["db"] else []))
    note("conv_wgrad", kind, shares)
    return max(shares.values())


@pytest.mark.parametrize("i", range(len(EXPECTED)), ids=[f"{i:02d}-{n}" for i, n in enumerate(EXPECTED)])
def test_recorded_step_replayed_vs_fp64(ops, i):
    calls, t0, out = recording(ops), time.time(), []
    n, r = calls[i]
    assert n == EXPECTED[i], (i, n)
    name = f"step[{i:02d}] {n}"
    if n == N_:
        c = dict(r)
        name += " " + R.case_id(c)
        for k, kind in enumerate(GN_KINDS):
            sh, _ = run_gn(ops, c, kind, "tagged" if (i + k) % 2 else "random", 500 + 11 * i + k, f"{name} {kind}")
            out.append(max(sh.values()))
    elif n == W_:
        name += f" {r['Cin']}->{r['Cout']} k{r['KH']} s{r['stride']} {r['H']}x{r['W']}" + (" strided dy" if r["dy_offset"] else "")
        out += [replay_wgrad(ops, r, kind, 600 + i, f"{name} {kind}") for kind in ("random", "tagged")]
    elif n == S_:
        out += [max(run_stem(ops, r["B"], r["H"], r["W"], r["Cout"], kind, r["db"], r["accumulate"], 700 + i, f"{name} {kind}").values())
                for kind in ("random", "tagged")]
    elif n == L_:
        name += f" {r['B'], r['N'], r['K']} {R.ACT_NAME[r['act_in']]}"
        out.append(max(run_linear(ops, r["B"], r["N"], r["K"], r["act_in"], r["db"], r["accumulate"], 800 + i, name).values()))
    else:
        gemms = GR.named([(m, [q]) for m, q in calls if m == M_])
        gi = [j for j, (m, _) in enumerate(calls) if m == M_].index(i)
        name += " " + gemms["names"][gi]
        for kind in GREF.KINDS:
            form, worst = GR.replay(ops, gemms, gemms["names"][gi], kind, 900 + i)
            FORMS_SEEN[gemms["names"][gi]] = form
            assert form != 0, (name, "form 0 at K = 3072")
            assert GEMM_FORM is None or form == GEMM_FORM, (name, form)
            WORST[("dgrad_2x2s2 gemm", "out", kind)] = max(WORST.get(("dgrad_2x2s2 gemm", "out", kind), 0.0), worst)
            out.append(worst)
    print(f"\n  {name}: {len(out)} replays ({time.time() - t0:.1f} s), worst share {max(out):.3f}")


# ---------------------------------------------------------------------------------------------------------------- (e) negative controls
def _rejected(fn, *needles):
    with pytest.raises(AssertionError) as e:
        fn()
    msg = str(e.value)
    for n in needles:
        assert n in msg, (n, msg)
    return msg


def test_negative_controls_on_real_kernel_output(ops):
    """a real kernel output against a deliberately wrong expectation: rejected, and the message names the element"""
    # eps 1e-5 where the kernel got 1e-6, on the const kind: a constant group with a small constant has r = 1 / sqrt(eps) and a tight bound
    c = dict(shape=(2, 70, 1024, 512), act=ACT_NONE, eps=1e-6, in_relu=False, pre=False, dx_in="sep", dw="plain")
    msg = _rejected(lambda: run_gn(ops, c, "const", "random", 41, "gn_bwd eps 1e-5 for 1e-6", expect_case=dict(c, eps=1e-5)),
                    "eps 1e-5 for 1e-6", "sample ", "pixel ", "channel ", "group ")
    assert int(msg.split("group ")[1].split(":")[0].split(",")[0]) % 3 != 2, msg            # a constant or nearly constant group
    print("\n  " + msg)
    # the expectation without the in_relu mask
    c = dict(shape=(2, 560, 256, 8), act=ACT_NONE, eps=1e-5, in_relu=True, pre=False, dx_in="none", dw="plain")
    msg = _rejected(lambda: run_gn(ops, c, "random", "random", 42, "gn_bwd no in_relu mask", expect_case=dict(c, in_relu=False)),
                    "no in_relu mask", "sample ", "pixel ", "channel ", "group ")
    print("  " + msg)
    # linear_wgrad: the expectation without the SiLU
    gen = torch.Generator(device=DEV).manual_seed(43)
    dy, x = torch.randn((3, 24), device=DEV, generator=gen), 3.0 * torch.randn((3, 16), device=DEV, generator=gen)
    dw = torch.empty((24, 16), device=DEV)
    ops.linear_wgrad(dy, x, dw, None, act_in=ACT_SILU)
    torch.cuda.synchronize()
    (ww, wb_), _ = R.linear_wgrad_expect(dy, x, ACT_SILU)
    R.check_vec("linear_wgrad right expectation", dw, ww, wb_, R.where_linear(16))
    (ww, wb_), _ = R.linear_wgrad_expect(dy, x, ACT_NONE)
    msg = _rejected(lambda: R.check_vec("linear_wgrad without the SiLU", dw, ww, wb_, R.where_linear(16)), "without the SiLU", "dw[n=", "][k=")
    print("  " + msg)


def test_print_worst():
    """(last: the tables over everything this module ran)"""
    print("\n  worst share of the allowance per kernel, output and operand kind:")
    for (kernel, out, kind), v in sorted(WORST.items()):
        print(f"    {kernel:18s} {out:5s} {kind:18s} {v:.3f}")
    print("  groupnorm_bwd dx: largest median share of the statistics' allowance in half an output ulp, per kind: " +
          ", ".join(f"{k} {v:.3g}" for k, v in STAT.items()))
    print(f"  dgrad_2x2s2 GEMM forms (last_gemm_tile): {FORMS_SEEN}")
    print("  groupnorm_bwd: reached per rows-per-block value:")
    for rows, what in sorted(REACHED.items()):
        print(f"    {rows:3d} rows: " + ", ".join(sorted(what)))
    if set(REACHED) >= {256, 32, 16, 8, 4, 2}:            # (the whole module ran)
        for rows, what in REACHED.items():
            assert {"in_relu", "pre_add+dpre", "dx_in sep", "dx_in alias"} <= what and set(GN_KINDS) <= what, (rows, sorted(what))
