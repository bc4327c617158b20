"""The Qwen2 prompt extension on the GPU (include/x2i_qwen_extend.h, Qwen2DecoderStack.extend, handoff.HipGenerate(keep_cache=True)): the two
kernels against the float64 checkers of tests/qwen_extend_ref.py and tests/qwen_ref.py with sentinel-filled surroundings, the attention's
two promises bit for bit, the stack against the library's float64 run over the whole prompt, and the hand-off over several calls."""
import pytest
import torch

from tests import qwen_decode_ref as DR
from tests import qwen_extend_ref as XR
from tests import qwen_ref as QR

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def qx():
    from x2i_amd import qwen_extend_ops as o
    o.load()
    return o


def _i32(v):
    return None if v is None else torch.tensor(v, dtype=torch.int32, device=DEV)


# ---------------------------------------------------------------------------------------------------------------- attention
def cache_inputs(B, Hq, Hkv, dk, cap, row0, n, seed, outside=0.0):
    """Q, K, V bf16 [B, H*, cap, dk] of tests/qwen_ref.py's kind in the slots < row0 + n; `outside`: what the slots from row0 + n on hold, and
    the rows of Q before row0"""
    S = row0 + n
    Q, K, V = QR.attention_inputs(B, Hq, Hkv, S, dk, seed=seed, Spad=cap, device=DEV)
    Q[:, :, :row0] = outside
    for t in (Q, K, V):
        t[:, :, S:] = outside
    return Q, K, V


def run_extend_attention(qx, Q, K, V, row0, n, k_lo=None, extra_cols=8, extra_rows=3):
    """-> (O [B, Hq, n, dk] view, the whole sentinel-filled output buffer [B, n + extra_rows, Hq * dk + extra_cols])"""
    B, Hq, cap, dk = Q.shape
    VT = V.transpose(-1, -2).contiguous()
    ldo = Hq * dk + extra_cols
    buf = XR.poisoned(B, n + extra_rows, ldo)
    qx.attention(Q, K, VT, buf, B, Hq, K.shape[1], row0, n, cap, dk, dk ** -0.5, ldo, (n + extra_rows) * ldo, _i32(k_lo))
    return buf[:, :n, :Hq * dk].reshape(B, n, Hq, dk).permute(0, 2, 1, 3), buf


def run_full_attention(Q, K, V, S, k_lo=None):
    """x2i_qwen_attention_bf16 on the same buffers with Spad = cap and k_hi = S -> O [B, Hq, S, dk]"""
    from x2i_amd import qwen_ops
    B, Hq, cap, dk = Q.shape
    VT = V.transpose(-1, -2).contiguous()
    buf = XR.poisoned(B, S, Hq * dk)
    lo = [0] * B if k_lo is None else k_lo
    qwen_ops.attention(Q, K, VT, buf, B, Hq, K.shape[1], S, cap, dk, dk ** -0.5, Hq * dk, S * Hq * dk, _i32(lo), _i32([S] * B))
    return buf.reshape(B, S, Hq, dk).permute(0, 2, 1, 3)


# (B, Hq, Hkv, dk, cap, row0, n, k_lo): one row; the last slot; aligned; row0 % 32 != 0 and the chunk crosses the 128-row block boundary; seven
# query heads per group over three blocks; a range that starts inside the chunk (rows 30..49 exactly 0)
ATTENTION_CASES = [(1, 1, 1, 128, 64, 1, 1, None), (1, 2, 2, 128, 192, 191, 1, None), (2, 4, 2, 128, 192, 64, 64, [0, 10]),
                   (1, 4, 2, 128, 256, 70, 61, None), (2, 14, 2, 64, 320, 129, 150, [0, 100]), (1, 2, 1, 128, 128, 30, 40, [50])]


@pytest.mark.parametrize("B,Hq,Hkv,dk,cap,row0,n,k_lo", ATTENTION_CASES)
def test_extend_attention_vs_fp64_per_tile(qx, B, Hq, Hkv, dk, cap, row0, n, k_lo):
    Q, K, V = cache_inputs(B, Hq, Hkv, dk, cap, row0, n, seed=1000 * row0 + n + dk)
    ref = XR.window_reference(Q, K, V, row0, n, dk ** -0.5, k_lo)
    O, buf = run_extend_attention(qx, Q, K, V, row0, n, k_lo)
    name = "qwen_extend_attention B=%d Hq=%d Hkv=%d dk=%d cap=%d rows %d..%d k_lo %s" % (B, Hq, Hkv, dk, cap, row0, row0 + n - 1, k_lo)
    worst = XR.check_window(name, O, ref, row0, k_lo)
    print("%s: worst tile rel-L2 %.3e (bound %.1e)" % (name, worst, QR.TOL_O))
    # exactly the n rows x Hq * dk columns are written
    assert bool(XR.is_sentinel(buf[:, n:]).all()) and bool(XR.is_sentinel(buf[:, :, Hq * dk:]).all())
    assert not bool(XR.is_sentinel(buf[:, :n, :Hq * dk]).any())
    # a relaunch is bit-identical
    O2, _ = run_extend_attention(qx, Q, K, V, row0, n, k_lo)
    assert torch.equal(O2, O)


# (..., first chunk row that must be bit-identical): every row where row0 % 32 == 0; rows >= 96 of the (70, 61) case, whose 32-row groups
# from 96 on hold no row below row0
IDENTITY_CASES = [(2, 4, 2, 128, 192, 64, 64, [0, 10], 64), (2, 14, 2, 64, 320, 128, 150, [0, 100], 128), (1, 4, 2, 128, 256, 70, 61, None, 96)]


@pytest.mark.parametrize("B,Hq,Hkv,dk,cap,row0,n,k_lo,first", IDENTITY_CASES)
def test_extend_attention_is_the_full_launch_bit_for_bit_where_the_geometry_is(qx, B, Hq, Hkv, dk, cap, row0, n, k_lo, first):
    """The same buffers through x2i_qwen_attention_bf16 with S = row0 + n, Spad = cap, k_hi = row0 + n.  (The buffers hold zeros outside
    the live slots: the full launch also reads the rows S .. of Q, which the extension never does -- include/x2i_qwen_extend.h.)"""
    Q, K, V = cache_inputs(B, Hq, Hkv, dk, cap, row0, n, seed=7 * row0 + n)
    O, _ = run_extend_attention(qx, Q, K, V, row0, n, k_lo)
    full = run_full_attention(Q, K, V, row0 + n, k_lo)
    assert torch.equal(O[:, :, first - row0:], full[:, :, first:])
    assert not bool(XR.is_sentinel(full).any())


@pytest.mark.parametrize("B,Hq,Hkv,dk,cap,row0,n,k_lo", [ATTENTION_CASES[3], ATTENTION_CASES[4]])
def test_extend_attention_is_a_function_of_live_data_only(qx, B, Hq, Hkv, dk, cap, row0, n, k_lo):
    """Everything that is not live -- the Q rows outside the chunk, K / V^T from row0 + n on and below k_lo -- overwritten by finite values of
    magnitude 1e30 with both signs: the output is bit-identical to the run with zeros there"""
    S = row0 + n
    Q, K, V = cache_inputs(B, Hq, Hkv, dk, cap, row0, n, seed=11 * row0 + n)
    for b, lo in enumerate(k_lo or [0] * B):
        K[b, :, :lo] = 0
        V[b, :, :lo] = 0
    O, _ = run_extend_attention(qx, Q, K, V, row0, n, k_lo)
    sign = lambda t: torch.where(torch.rand(t.shape, generator=torch.Generator().manual_seed(5)).to(DEV) < 0.5, -1e30, 1e30).to(torch.bfloat16)
    Q2, K2, V2 = Q.clone(), K.clone(), V.clone()
    Q2[:, :, :row0] = sign(Q2[:, :, :row0])
    Q2[:, :, S:] = sign(Q2[:, :, S:])
    for t in (K2, V2):
        t[:, :, S:] = sign(t[:, :, S:])
        for b, lo in enumerate(k_lo or [0] * B):
            t[b, :, :lo] = sign(t[b, :, :lo])
    assert bool(torch.isfinite(Q2).all()) and float(Q2[:, :, :row0].abs().min()) > 9e29
    O2, _ = run_extend_attention(qx, Q2, K2, V2, row0, n, k_lo)
    assert torch.equal(O2, O)
    XR.check_window("qwen_extend_attention, 1e30 outside", O2, XR.window_reference(Q, K, V, row0, n, dk ** -0.5, k_lo), row0, k_lo)


def test_extend_attention_refusals(qx):
    from x2i_amd._lib import X2IError
    Q, K, V = cache_inputs(1, 4, 2, 128, 64, 5, 3, seed=1)
    VT = V.transpose(-1, -2).contiguous()
    out = XR.poisoned(1, 3, 512)
    call = lambda Hq=4, Hkv=2, row0=5, n=3, cap=64, dk=128, scale=0.1, ldo=512: qx.attention(Q, K, VT, out, 1, Hq, Hkv, row0, n, cap, dk, scale, ldo,
                                                                                             3 * 512)
    for bad in (dict(dk=32), dict(Hq=3), dict(cap=40), dict(row0=-1), dict(n=0), dict(row0=62), dict(scale=0.0), dict(ldo=510)):
        with pytest.raises(X2IError):
            call(**bad)
    assert bool(XR.is_sentinel(out).all())     # refused before any launch


# ---------------------------------------------------------------------------------------------------------------- RoPE + head split
CAP = 192
# (row0, n): one row at slot 0; inside one 16-byte column group; straddling a group; two 64-boundaries with a ragged head and tail; aligned;
# the last slot
ROPE_WINDOWS = [(0, 1), (5, 3), (7, 2), (61, 70), (64, 64), (CAP - 1, 1)]


@pytest.mark.parametrize("row0,n", ROPE_WINDOWS)
@pytest.mark.parametrize("B,Hq,Hkv,dk,mrope", [(1, 4, 2, 128, False), (3, 14, 2, 64, True)])
def test_extend_rope_split_vs_fp64_and_writes_nothing_else(qx, B, Hq, Hkv, dk, mrope, row0, n):
    """Tables from rope_tables at positions that are not the slots.  q and k per element against float64 from the same f32 tables; the V^T
    columns bit-equal to the torch transposition; every element of Q, K, VT outside the chunk's rows / columns still the sentinel; the row
    stride honoured; and the rows are those of x2i_qwen_rope_split_bf16, bit for bit."""
    from x2i_amd import qwen_ops
    from x2i_amd.qwen import rope_tables
    g = torch.Generator().manual_seed(row0 * 100 + n + dk)
    if mrope:
        pos, sec = QR.mrope_positions(B, n, seed=n) + 1000, ([16, 24, 24] if dk == 128 else [8, 12, 12])
    else:
        pos, sec = torch.randint(0, 4001, (B, n), generator=g), None
    cos, sin = rope_tables(pos.to(DEV), dk, 1000000.0, sec)
    W, ld = (Hq + 2 * Hkv) * dk, (Hq + 2 * Hkv) * dk + 16
    qkv = torch.zeros((B * n, ld), dtype=torch.bfloat16, device=DEV)
    qkv[:, :W] = (2.0 * torch.randn((B * n, W), generator=g)).bfloat16().to(DEV)
    Q, K, VT = XR.poisoned(B, Hq, CAP, dk), XR.poisoned(B, Hkv, CAP, dk), XR.poisoned(B, Hkv, dk, CAP)
    qx.rope_split(qkv, cos, sin, Q, K, VT, B, row0, n, CAP, Hq, Hkv, dk)
    q, k, v = (t.reshape(B, n, -1, dk) for t in qkv[:, :W].view(B, n, W).split([Hq * dk, Hkv * dk, Hkv * dk], dim=-1))
    sl = slice(row0, row0 + n)
    eq = QR.check_rope("qwen_extend_rope_split q", Q[:, :, sl].transpose(1, 2), q, cos, sin)
    ek = QR.check_rope("qwen_extend_rope_split k", K[:, :, sl].transpose(1, 2), k, cos, sin)
    print("qwen_extend_rope_split B=%d Hq=%d Hkv=%d dk=%d rows %d..%d: worst error / bound q %.3f k %.3f" % (B, Hq, Hkv, dk, row0, row0 + n - 1, eq, ek))
    assert torch.equal(VT[:, :, :, sl], v.permute(0, 2, 3, 1))                              # V is exact
    for t, dim in ((Q, 2), (K, 2), (VT, 3)):
        rest = torch.cat((t.narrow(dim, 0, row0), t.narrow(dim, row0 + n, CAP - row0 - n)), dim)
        assert bool(XR.is_sentinel(rest).all())
    # the prefill kernel's rows at slot 0 .. n - 1 are these rows
    Spad = qwen_ops.pad64(n)
    Q0, K0, VT0 = XR.poisoned(B, Hq, Spad, dk), XR.poisoned(B, Hkv, Spad, dk), XR.poisoned(B, Hkv, dk, Spad)
    qwen_ops.rope_split(qkv, cos, sin, Q0, K0, VT0, B, n, Spad, Hq, Hkv, dk)
    assert torch.equal(Q[:, :, sl], Q0[:, :, :n]) and torch.equal(K[:, :, sl], K0[:, :, :n]) and torch.equal(VT[:, :, :, sl], VT0[:, :, :, :n])


def test_extend_rope_split_refusals(qx):
    from x2i_amd._lib import X2IError
    B, Hq, Hkv, dk, n = 1, 2, 1, 128, 3
    qkv = torch.zeros((n, 4 * dk), dtype=torch.bfloat16, device=DEV)
    cos = torch.ones((B, n, dk // 2), device=DEV)
    Q, K, VT = XR.poisoned(B, Hq, 64, dk), XR.poisoned(B, Hkv, 64, dk), XR.poisoned(B, Hkv, dk, 64)
    call = lambda row0=5, n=n, cap=64, dk=dk, ld=None: qx.rope_split(qkv, cos, cos, Q, K, VT, B, row0, n, cap, Hq, Hkv, dk, ld=ld)
    for bad in (dict(row0=-1), dict(row0=62), dict(cap=72), dict(ld=4 * dk - 8), dict(ld=4 * dk + 4)):
        with pytest.raises(X2IError):
            call(**bad)
    with pytest.raises(X2IError):
        qx.rope_split(qkv, cos[:, :2], cos[:, :2], Q, K, VT, B, 5, n, 64, Hq, Hkv, dk)        # tables of another chunk
    assert all(bool(XR.is_sentinel(t).all()) for t in (Q, K, VT))


# ---------------------------------------------------------------------------------------------------------------- the stack
def _library_rows(m, x, pos, dev, dt):
    out = m(inputs_embeds=x.to(device=dev, dtype=dt), attention_mask=None, position_ids=pos.to(dev), output_hidden_states=True, use_cache=False)
    return torch.stack(tuple(out.hidden_states), 1)


def _stacks(hidden, Hq, Hkv, d_ff, layers, vl, seed):
    from x2i_amd.qwen import Qwen2DecoderStack
    cfg, lib = QR.library_stack(hidden, Hq, Hkv, d_ff, layers, vl=vl)
    sd = QR.random_stack_state_dict(lib, seed=seed)
    lib.load_state_dict(sd, strict=True)
    hip = Qwen2DecoderStack(cfg, device="cpu")
    hip.load_state_dict({k: v.bfloat16() for k, v in sd.items()}, strict=True)
    return lib, hip.to(DEV)


def _criterion(name, got, lib_bf16, ref):
    e_hip, e_lib = QR.rel_l2(got, ref), QR.rel_l2(lib_bf16, ref)
    print("%s: rel-L2 against float64: HIP %.3e, transformers bf16 on the GPU %.3e (ratio %.2f)" % (name, e_hip, e_lib, e_hip / e_lib))
    XR.assert_stack_criterion(e_hip, e_lib)


T_STEPS = 2
# (hidden, Hq, Hkv, d_ff, layers, B, S, P, vl): the two configurations of tests/test_qwen_decode_gpu.py's DECODE_CASES without padding; the
# first P rows are prefilled, the rest is the extension (P = 70: the chunk starts inside a wave and crosses the 128-row block boundary)
STACK_CASES = [(512, 4, 2, 1024, 2, 2, 130, 70, False), (256, 2, 1, 512, 2, 2, 77, 33, True)]


@pytest.mark.parametrize("hidden,Hq,Hkv,d_ff,layers,B,S,P,vl", STACK_CASES)
def test_extend_and_decode_steps_vs_library_fp64_and_bf16(hidden, Hq, Hkv, d_ff, layers, B, S, P, vl):
    lib, hip = _stacks(hidden, Hq, Hkv, d_ff, layers, vl, seed=hidden + S)
    T, n = T_STEPS, S - P
    g = torch.Generator().manual_seed(S)
    x = torch.randn((B, S, hidden), generator=g).bfloat16()
    steps = torch.randn((B, T, hidden), generator=g).bfloat16()
    pos = QR.mrope_positions(B, S, seed=S) if vl else torch.arange(S)[None].expand(B, S)
    dev = lambda t: t.to(DEV)
    cache = hip.new_cache(B, S + T)
    hip.prefill(cache, inputs_embeds=dev(x[:, :P]), position_ids=dev(pos[..., :P]))
    K0, VT0 = cache.K.clone(), cache.VT.clone()
    new = hip.extend(cache, P, inputs_embeds=dev(x[:, P:]), position_ids=dev(pos[..., P:]))
    assert new.shape == (B, layers + 1, n, hidden) and new.dtype == torch.bfloat16 and torch.equal(new[:, 0], dev(x[:, P:]))
    # the cache afterwards
    nxt = DR.next_positions(pos[..., P:], None)
    assert cache.k_lo.tolist() == [0] * B and cache.k_hi.tolist() == [S] * B and cache.steps == S
    assert torch.equal(cache.pos.cpu(), nxt.expand_as(cache.pos))
    assert torch.equal(cache.K[:, :, :, :P], K0[:, :, :, :P]) and torch.equal(cache.VT[..., :P], VT0[..., :P])       # the kept slots
    assert torch.equal(cache.K[:, :, :, S:], K0[:, :, :, S:]) and torch.equal(cache.VT[..., S:], VT0[..., S:])       # nothing past the chunk
    assert bool((cache.K[:, :, :, P:S] != 0).any(-1).all()) and bool((cache.VT[..., P:S] != 0).any(-2).all())        # every slot of the chunk
    # ... and a prompt-shaped call of another length beside it does not evict the extension's workspace, nor the other way round
    ws_p, ws_x = hip._ws, hip._xws
    assert (B, P) in ws_p and (B, n) in ws_x
    # two teacher-forced steps
    answer = XR.poisoned(B, layers + 1, T, hidden)
    for t in range(T):
        hip.decode_step(cache, inputs_embeds=dev(steps[:, t:t + 1]), out=answer[:, :, t])
    assert cache.k_hi.tolist() == [S + T] * B and hip._ws is ws_p and hip._xws is ws_x
    # against the library: ONE causal pass over the whole prompt and the steps
    xcat = torch.cat((x, steps), 1)
    pcat = torch.cat((pos, DR.step_positions(nxt, T).expand(*pos.shape[:-1], T)), -1)
    name = "extend hidden=%d %dq/%dkv layers=%d B=%d S=%d keep=%d vl=%s" % (hidden, Hq, Hkv, layers, B, S, P, vl)
    ref = _library_rows(lib.double(), xcat, pcat, "cpu", torch.float64)
    lib_bf16 = _library_rows(lib.to(device=DEV, dtype=torch.bfloat16), xcat, pcat, DEV, torch.bfloat16)
    _criterion(name + ", the chunk's rows", new, lib_bf16[:, :, P:S], ref[:, :, P:S])
    _criterion(name + ", two decode steps after it", answer, lib_bf16[:, :, S:], ref[:, :, S:])


def test_extend_truncates_what_the_cache_held_and_a_captured_step_replays():
    """prefill 130 rows, six decode steps (one eager, five replays of a step captured on the cache), then extend(keep=100) with 30 OTHER rows:
    what slots 100 .. 135 held is dropped.  The chunk's rows and one more step, replayed from the graph captured BEFORE the extension, against
    the library on the 100 + 30 (+ 1) sequence; the replay is the eager step bit for bit."""
    hidden, Hq, Hkv, d_ff, layers, B, S, keep, n = 512, 4, 2, 1024, 2, 2, 130, 100, 30
    lib, hip = _stacks(hidden, Hq, Hkv, d_ff, layers, False, seed=77)
    g = torch.Generator().manual_seed(8)
    x = torch.randn((B, S, hidden), generator=g).bfloat16().to(DEV)
    steps = torch.randn((B, 7, hidden), generator=g).bfloat16().to(DEV)
    other = torch.randn((B, n, hidden), generator=g).bfloat16().to(DEV)
    cache = hip.new_cache(B, S + 8)
    hip.prefill(cache, inputs_embeds=x, position_ids=torch.arange(S, device=DEV)[None].expand(B, S))
    static_x = torch.zeros((B, 1, hidden), device=DEV, dtype=torch.bfloat16)
    static_out = torch.zeros((B, layers + 1, hidden), device=DEV, dtype=torch.bfloat16)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        static_x.copy_(steps[:, 0:1])
        hip.decode_step(cache, inputs_embeds=static_x, out=static_out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.decode_step(cache, inputs_embeds=static_x, out=static_out)
    cache.steps -= 1                                          # (a capture runs nothing)
    for t in range(1, 6):
        static_x.copy_(steps[:, t:t + 1])
        graph.replay()
        cache.steps += 1
    assert cache.k_hi.tolist() == [S + 6] * B and cache.steps == S + 6
    pos = torch.arange(keep, keep + n, device=DEV)[None].expand(B, n)
    new = hip.extend(cache, keep, inputs_embeds=other, position_ids=pos)
    assert cache.k_hi.tolist() == [keep + n] * B and cache.pos.tolist() == [keep + n] * B and cache.steps == keep + n
    snap = [t.clone() for t in (cache.K, cache.VT, cache.k_hi, cache.pos)]
    static_x.copy_(steps[:, 6:7])
    graph.replay()
    replayed = static_out.clone()
    assert cache.k_hi.tolist() == [keep + n + 1] * B
    for dst, src in zip((cache.K, cache.VT, cache.k_hi, cache.pos), snap):
        dst.copy_(src)
    eager = hip.decode_step(cache, inputs_embeds=steps[:, 6:7])
    assert torch.equal(eager[:, :, 0], replayed)
    xcat = torch.cat((x[:, :keep], other, steps[:, 6:7]), 1).cpu()
    pcat = torch.arange(keep + n + 1)[None].expand(B, keep + n + 1)
    ref = _library_rows(lib.double(), xcat, pcat, "cpu", torch.float64)
    lib_bf16 = _library_rows(lib.to(device=DEV, dtype=torch.bfloat16), xcat, pcat, DEV, torch.bfloat16)
    _criterion("extend(keep=100) after 130 + 6, the chunk's rows", new, lib_bf16[:, :, keep:keep + n], ref[:, :, keep:keep + n])
    _criterion("extend(keep=100) after 130 + 6, a replayed step", replayed.unsqueeze(2), lib_bf16[:, :, keep + n:], ref[:, :, keep + n:])


def test_extend_refuses_a_hole_a_full_and_a_foreign_cache():
    from x2i_amd.qwen import Qwen2DecoderStack
    kw = dict(hidden_size=256, num_attention_heads=2, num_key_value_heads=1, intermediate_size=512, num_hidden_layers=1, vocab_size=64, device=DEV)
    hip, other = Qwen2DecoderStack(**kw).init_random_(1), Qwen2DecoderStack(**kw).init_random_(2)
    B, S = 2, 77
    ids = torch.randint(0, 64, (B, S), generator=torch.Generator().manual_seed(3)).to(DEV)
    mask = torch.ones((B, S), dtype=torch.long, device=DEV)
    mask[0, 50:] = 0
    cache = hip.new_cache(B, 100)                             # cap 128
    hip.prefill(cache, input_ids=ids, attention_mask=mask)
    pos = lambda a, n: torch.arange(a, a + n, device=DEV)[None].expand(B, n)
    K0 = cache.K.clone()
    with pytest.raises(ValueError, match="hole"):
        hip.extend(cache, 60, input_ids=ids[:, :5], position_ids=pos(60, 5))               # sample 0's keys end at 50
    with pytest.raises(ValueError, match="cap"):
        hip.extend(cache, 50, input_ids=torch.cat((ids, ids), 1)[:, :78], position_ids=pos(50, 78))       # 50 + 78 + 1 > 128
    with pytest.raises(ValueError, match="new_cache"):
        other.extend(cache, 50, input_ids=ids[:, :5], position_ids=pos(50, 5))
    assert torch.equal(cache.K, K0) and cache.k_hi.tolist() == [50, 77] and cache.steps == S
    out = hip.extend(cache, 50, input_ids=ids[:, :5], position_ids=pos(50, 5))              # ... and keep = 50 is none of these
    assert out.shape == (B, 2, 5, 256) and cache.k_hi.tolist() == [55, 55]
    assert torch.equal(out[:, 0], hip.embed_tokens.weight[ids[:, :5]])


# ---------------------------------------------------------------------------------------------------------------- hand-off
SEED = 5


def tiny_model():
    """The tiny random Qwen2ForCausalLM of tests/test_qwen_decode_gpu.py's hand-off test (hidden 256, 2 heads of 128, 1 kv head, 3 layers)"""
    from transformers import Qwen2ForCausalLM
    cfg = QR.library_config(256, 2, 1, 512, 3)
    cfg._attn_implementation = "sdpa"
    torch.manual_seed(0)
    model = Qwen2ForCausalLM(cfg).eval().requires_grad_(False)
    model.model.load_state_dict(QR.random_stack_state_dict(model.model, seed=SEED), strict=True)
    return model.to(device=DEV, dtype=torch.bfloat16)


def _library_slab(decoder, ids, dev, dt):
    import copy
    m = copy.deepcopy(decoder).to(device=dev, dtype=dt)
    return torch.stack(tuple(m(input_ids=ids.to(dev), output_hidden_states=True, use_cache=False).hidden_states), 1)


def check_call(model, out, ids, procs, hip_head, name):
    """What every call must satisfy: the prompt slab meets the stack criterion against the library over the WHOLE prompt, every returned token
    is the argmax of the lm_head (with the processor) over the returned state before it, and the decoder's forward is restored"""
    from tests import qwen_head_ref as HR
    from x2i_amd.handoff import find_decoder
    S = ids.shape[1]
    T = out.sequences.shape[1] - S
    assert "forward" not in find_decoder(model).__dict__
    assert out.prompt.shape[2] == S and torch.equal(out.sequences[:, :S], ids) and out.answer.shape[2] == T - 1
    ref = _library_slab(model.model, ids, "cpu", torch.float64)
    _criterion(name, out.prompt, _library_slab(model.model, ids, DEV, torch.bfloat16), ref)
    for t in range(T):
        x = out.prompt[:, -1, S - 1] if t == 0 else out.answer[:, -1, t - 1]
        if hip_head:
            want, bound, _ = HR.head_expect(x, model.lm_head.weight, HR.seen_of(out.sequences[:, :S + t], 64), 1.05)
            gap, allow = HR.margin(want, bound)
            assert bool((gap > allow).all()), "seed %d, token %d: the float64 margin %s does not exceed twice the bound %s -- an unlucky " \
                "seed, not a wrong token: choose another" % (SEED, t, gap.tolist(), allow.tolist())
            assert torch.equal(HR.argmax_lowest(want), out.sequences[:, S + t]), t
        else:
            first = model.lm_head(out.prompt[:, -1])[:, S - 1]      # (token 0 through the lm_head call of the shape the model itself makes)
            scores = procs[0](out.sequences[:, :S + t], (first if t == 0 else model.lm_head(x)).float())
            assert torch.equal(scores.argmax(-1), out.sequences[:, S + t]), t
    assert torch.equal(out.answer[:, 0], model.model.embed_tokens.weight[out.sequences[:, S:S + T - 1]])


def same(a, b):
    return all(torch.equal(getattr(a, f), getattr(b, f)) for f in ("prompt", "answer", "sequences", "lengths"))


@pytest.mark.parametrize("graph,hip_head", [(False, False), (True, False), (True, True)])
def test_hip_generate_keeps_its_cache_between_calls(graph, hip_head):
    from transformers.generation.logits_process import RepetitionPenaltyLogitsProcessor
    from x2i_amd.handoff import HipGenerate
    model = tiny_model()
    procs = [RepetitionPenaltyLogitsProcessor(1.05)]
    S, T = 77, 9
    g = torch.Generator().manual_seed(6)
    ids1 = torch.randint(0, 64, (1, S), generator=g).to(DEV)
    more = torch.randint(0, 64, (1, 1020), generator=g).to(DEV)
    kw = dict(max_new_tokens=T, eos_token_id=None, logits_processor=procs, graph=graph)
    hg, plain = HipGenerate(model, hip_head=hip_head, keep_cache=True), HipGenerate(model, hip_head=hip_head)
    assert hg.reused == 0
    # call 1: a whole prefill, bit for bit what an instance without the flag returns
    out1 = hg.generate(model, input_ids=ids1, **kw)
    assert hg.reused == 0 and same(out1, plain.generate(model, input_ids=ids1, **kw)) and out1.lengths.tolist() == [T]
    kept = torch.cat((out1.prompt, out1.answer), 2)
    cap1 = hg._state["cache"].cap
    assert cap1 == 1024 and plain._state["cache"].cap == 128
    # call 2: call 1's sequences and 20 new ids; everything but the last generated token's pass is there
    ids2 = torch.cat((out1.sequences, more[:, :20]), 1)
    out2 = hg.generate(model, input_ids=ids2, attention_mask=torch.ones_like(ids2), **kw)
    assert hg.reused == S + T - 1 and hg.reuse_note == "" and out2.prompt.shape[2] == S + T + 20 and hg._state["cache"].cap == cap1
    assert torch.equal(out2.prompt[:, :, :hg.reused], kept)
    check_call(model, out2, ids2, procs, hip_head, "keep_cache call 2 (graph=%s hip_head=%s), reused %d of %d" % (graph, hip_head, hg.reused, S + T + 20))

    # call 1's prompt again: it is a prefix of what is kept, nothing new stands after it, so it is a whole prefill -- with call 1's bits
    out = hg.generate(model, input_ids=ids1, **kw)
    assert hg.reused == 0 and "nothing new" in hg.reuse_note and same(out, out1)

    def again():      # the state after call 1
        hg.forget()
        assert same(hg.generate(model, input_ids=ids1, **kw), out1) and hg.reused == 0

    # id 40 changed: the prefix ends there
    ids = ids2.clone()
    ids[0, 40] = (ids[0, 40] + 1) % 64
    out = hg.generate(model, input_ids=ids, **kw)
    assert hg.reused == 40 and torch.equal(out.prompt[:, :, :40], kept[:, :, :40])
    check_call(model, out, ids, procs, hip_head, "keep_cache, id 40 changed, reused 40")
    # id 0 changed: nothing in common, and the result is a fresh instance's bit for bit
    again()
    ids = ids2.clone()
    ids[0, 0] = (ids[0, 0] + 1) % 64
    out = hg.generate(model, input_ids=ids, **kw)
    assert hg.reused == 0 and "no common prefix" in hg.reuse_note and same(out, HipGenerate(model, hip_head=hip_head).generate(model, input_ids=ids, **kw))
    # a padded mask: a whole prefill
    again()
    mask = torch.ones_like(ids2)
    mask[0, :3] = 0
    hg.generate(model, input_ids=ids2, attention_mask=mask, **kw)
    assert hg.reused == 0 and "padded" in hg.reuse_note
    hg.generate(model, input_ids=torch.cat((ids2, more[:, 20:25]), 1), **kw)             # ... and so is the call after a padded one
    assert hg.reused == 0 and "padded" in hg.reuse_note
    # a turn that outgrows the capacity is still reused, on a larger cache
    again()
    ids = torch.cat((out1.sequences, more), 1)
    out = hg.generate(model, input_ids=ids, **kw)
    assert hg.reused == S + T - 1 and hg._state["cache"].cap == 2048 and torch.equal(out.prompt[:, :, :hg.reused], kept)
    check_call(model, out, ids, procs, hip_head, "keep_cache, a turn of %d tokens on a larger cache, reused %d" % (ids.shape[1], hg.reused))
    # forget() drops the conversation
    again()
    hg.forget()
    hg.generate(model, input_ids=ids2, **kw)
    assert hg.reused == 0 and "no kept conversation" in hg.reuse_note
    # a call that fails inside the prompt pass leaves no conversation behind: its prefill may have rewritten the cache
    again()
    hole = torch.ones_like(ids2)
    hole[0, 10] = 0
    with pytest.raises(ValueError, match="contiguous"):
        hg.generate(model, input_ids=ids2, attention_mask=hole, **kw)
    hg.generate(model, input_ids=ids2, **kw)
    assert hg.reused == 0 and "no kept conversation" in hg.reuse_note
    # per call: keep_cache=False on this instance is a call of today, and drops the conversation too
    assert same(hg.generate(model, input_ids=ids1, keep_cache=False, **kw), plain.generate(model, input_ids=ids1, **kw))
    assert hg._state["cache"].cap == 128 and hg._conv is None


class StubProcessor:
    """a tokenizer of 60 words for the multi-turn conditioner (tests/test_qwen_head_gpu.py's): ids 2 .. 61 are the 'words' w2 .. w61, a turn
    of the history is its words"""

    def apply_chat_template(self, history, tokenize=False, add_generation_prompt=True):
        return " | ".join(c["text"] for m in history for c in m["content"] if c["type"] == "text")

    def __call__(self, text, images=None, return_tensors="pt"):
        from transformers import BatchFeature
        ids = [[int(w[1:]) for w in t.replace("|", " ").split()] for t in text]
        return BatchFeature({"input_ids": torch.tensor(ids), "attention_mask": torch.ones((len(ids), len(ids[0])), dtype=torch.long)})

    def batch_decode(self, ids, skip_special_tokens=True):
        return [" ".join("w%d" % min(max(int(i), 2), 61) for i in row) for row in ids]


def test_multi_turn_conditioner_keeps_the_cache_over_three_turns():
    from transformers import GenerationConfig
    from x2i_amd.infer.inference_multi_turn import MultiTurnConditioner
    model = tiny_model()
    model.generation_config = GenerationConfig(do_sample=True, top_k=1, temperature=0.5, repetition_penalty=1.05, eos_token_id=1, pad_token_id=0)
    cond = MultiTurnConditioner(None, DEV, hip_generate=True, keep_cache=True, model=model, processor=StubProcessor())
    assert cond.generate.keep_cache is True
    text, reused, last = [], [], None
    for turn, p in enumerate(["w5 w9 w33 w12 w7 w40 w21", "w3 w3 w8", "w17 w2 w44 w9"]):
        slab, answer = cond(text_prompt=p)
        text.append(p)
        ids = StubProcessor()([" | ".join(text)])["input_ids"].to(DEV)
        S, n = ids.shape[1], len(answer.split())
        assert slab.shape == (1, 4, S + n - 1, 256)                 # the full prompt and the answer's passes
        reused.append(cond.generate.reused)
        if last is not None:
            assert torch.equal(slab[:, :, :reused[-1]], last[:, :, :reused[-1]])
        _criterion("multi-turn turn %d, prompt of %d, reused %d" % (turn, S, reused[-1]), slab[:, :, :S],
                   _library_slab(model.model, ids, DEV, torch.bfloat16), _library_slab(model.model, ids, "cpu", torch.float64))
        text.append(answer)
        last = slab
    assert reused[0] == 0 and 7 <= reused[1] < reused[2], reused
    with pytest.raises(ValueError, match="--hip_keep_cache.*--hip_generate"):
        MultiTurnConditioner(None, DEV, keep_cache=True, model=model, processor=StubProcessor())
