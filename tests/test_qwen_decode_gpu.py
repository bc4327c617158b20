"""GPU checks of Qwen2 decoding with a key/value cache (include/x2i_qwen_decode.h, Qwen2DecoderStack.new_cache / prefill / decode_step): the
three entry points against float64 per row / per element with sentinel-filled surroundings, their bit-level promises (relaunch, batch
independence), and the stack's prefill and teacher-forced decode steps against the library in float64 and in bf16 on the same GPU."""
import pytest
import torch

from tests import attn_ref
from tests import gemm_ref as G
from tests import qwen_decode_ref as DR
from tests import qwen_ref as QR
from tests.test_t5_gpu import assert_stack_criterion, is_sentinel, poisoned  # (helpers; its tests are not re-collected here)

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def qd():
    from x2i_amd import qwen_decode_ops as o
    o.load()
    return o


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


# ---------------------------------------------------------------------------------------------------------------- attention
def decode_inputs(B, Hq, Hkv, dk, cap, seed):
    """q, k ~ 1.5 N(0, 1), v ~ N(0, 1) (qwen_ref.attention_inputs' scales) over the WHOLE cache: the keys outside a range are live values"""
    g = torch.Generator().manual_seed(seed)
    q = (1.5 * torch.randn((B, Hq, dk), generator=g)).bfloat16().to(DEV)
    k = (1.5 * torch.randn((B, Hkv, cap, dk), generator=g)).bfloat16().to(DEV)
    v = torch.randn((B, Hkv, cap, dk), generator=g).bfloat16().to(DEV)
    return q, k, v


def run_decode_attention(qd, Qd, K, V, k_lo, k_hi, extra_cols=8):
    """-> (O [B, Hq, dk] view, the whole sentinel-filled output buffer [B, Hq * dk + extra_cols])"""
    B, Hq, dk = Qd.shape
    Hkv, cap = K.shape[1], K.shape[2]
    VT = V.transpose(-1, -2).contiguous()
    buf = poisoned(B, Hq * dk + extra_cols)
    ws = torch.full((qd.workspace_floats(B, Hq, cap, dk),), float("nan"), device=DEV)       # its contents before a call are irrelevant
    qd.attention(Qd, K, VT, _i32(k_lo), _i32(k_hi), buf, ws, B, Hq, Hkv, cap, dk, dk ** -0.5)
    return buf[:, :Hq * dk].view(B, Hq, dk), buf


def check_rows(name, O, ref):
    """every (b, h) row within TOL_O (rel-L2): the rows as one-row tiles of attn_ref.check_tiles"""
    return attn_ref.check_tiles(name, O[:, :, None], ref[:, :, None], QR.TOL_O)


# (B, Hq, Hkv, dk, cap, k_lo, k_hi): one key; two samples ending before / on a tile edge; a group of seven heads of 64 with left padding; a
# range that crosses a chunk edge; four chunks with a group of eight; a start on a tile edge and a single last key; empty ranges
# Worst row measured on the MI355X, in this order: 0, 1.98e-3, 2.38e-3, 2.44e-3, 2.14e-3, 1.72e-3, 0 (bound TOL_O = 5e-3)
ATTENTION_CASES = [(1, 1, 1, 128, 64, [0], [1]), (2, 4, 2, 128, 128, [0, 0], [63, 64]), (2, 14, 2, 64, 192, [0, 70], [65, 130]),
                   (1, 7, 1, 128, 320, [0], [300]), (1, 16, 2, 128, 1024, [5], [1000]), (2, 2, 2, 128, 128, [64, 127], [128, 128]),
                   (2, 4, 2, 128, 128, [5, 100], [5, 90])]


@pytest.mark.parametrize("B,Hq,Hkv,dk,cap,k_lo,k_hi", ATTENTION_CASES)
def test_decode_attention_vs_fp64(qd, B, Hq, Hkv, dk, cap, k_lo, k_hi):
    Qd, K, V = decode_inputs(B, Hq, Hkv, dk, cap, seed=cap + Hq)
    ref = DR.attention_reference(Qd, K, V, k_lo, k_hi, dk ** -0.5)
    O, buf = run_decode_attention(qd, Qd, K, V, k_lo, k_hi)
    worst = check_rows("decode_attention %s" % ((B, Hq, Hkv, dk, cap, k_lo, k_hi),), O, ref)
    print("decode_attention %s: worst row rel-L2 %.3e (bound %.1e)" % ((B, Hq, Hkv, dk, cap, k_lo, k_hi), worst, QR.TOL_O))
    assert bool(is_sentinel(buf[:, Hq * dk:]).all())                     # the padding of the output rows is untouched
    for b in range(B):
        if k_hi[b] <= k_lo[b]:
            assert bool((O[b].view(torch.int16) == 0).all())            # an empty range: exactly 0, and written
    O2, _ = run_decode_attention(qd, Qd, K, V, k_lo, k_hi)
    assert torch.equal(O2, O)                                            # a relaunch is bit-identical
    O0, _ = run_decode_attention(qd, Qd[:1].contiguous(), K[:1].contiguous(), V[:1].contiguous(), k_lo[:1], k_hi[:1])
    assert torch.equal(O0[0], O[0])                                      # sample 0 alone and in its batch


def test_decode_attention_clamps_its_ranges(qd):
    Qd, K, V = decode_inputs(2, 4, 2, 128, 128, seed=3)
    O, _ = run_decode_attention(qd, Qd, K, V, [-7, 100], [90, 4000])
    O2, _ = run_decode_attention(qd, Qd, K, V, [0, 100], [90, 128])
    assert torch.equal(O, O2)
    check_rows("decode_attention clamped", O, DR.attention_reference(Qd, K, V, [-7, 100], [90, 4000], 128 ** -0.5))


@pytest.mark.parametrize("cap,k_lo,k_hi", [(128, [30], [90]), (576, [200], [530])])
def test_decode_attention_masks_by_index_under_adversarial_magnitudes(qd, cap, k_lo, k_hi):
    """The construction of tests/test_qwen_gpu.py's test of the same name: q and the counted keys shifted along one shared unit direction u
    by c with c^2 / sqrt(128) = 9, so that every counted pair loses 9; every key outside the range holds -c u and scores near +9, with V = 50
    there.  Then the contents outside the range change, and the result must not."""
    B, Hq, Hkv, dk = 1, 2, 1, 128
    c = (9.0 * dk ** 0.5) ** 0.5
    Qd, K, V = decode_inputs(B, Hq, Hkv, dk, cap, seed=7)
    u = torch.randn((B, Hkv, 1, dk), generator=torch.Generator().manual_seed(8)).to(DEV)
    u /= u.norm(dim=-1, keepdim=True)
    lo, hi = k_lo[0], k_hi[0]
    Qd[:] = (Qd.float() - c * u[:, :, 0].repeat_interleave(Hq // Hkv, dim=1)).bfloat16()
    K[:, :, lo:hi] = (K[:, :, lo:hi].float() + c * u).bfloat16()
    for sl in (slice(0, lo), slice(hi, None)):
        K[:, :, sl] = (-c * u).bfloat16()
        V[:, :, sl] = 50.0
    O, _ = run_decode_attention(qd, Qd, K, V, k_lo, k_hi)
    check_rows("decode_attention anti", O, DR.attention_reference(Qd, K, V, k_lo, k_hi, dk ** -0.5))
    K2, V2 = K.clone(), V.clone()
    for sl in (slice(0, lo), slice(hi, None)):
        K2[:, :, sl] = (3.0 * c * u).bfloat16()
        V2[:, :, sl] = -1000.0
    O2, _ = run_decode_attention(qd, Qd, K2, V2, k_lo, k_hi)
    assert torch.equal(O2, O)


# ---------------------------------------------------------------------------------------------------------------- rope_append
@pytest.mark.parametrize("B,Hq,Hkv,dk,cap,slots", [(1, 1, 1, 128, 64, [0]), (3, 4, 2, 128, 128, [127, 5, 64]), (2, 14, 2, 64, 192, [191, 70]),
                                                   (3, 2, 1, 128, 64, [64, 7, -1])])
def test_rope_append_vs_fp64_and_writes_nothing_else(qd, B, Hq, Hkv, dk, cap, slots):
    """q and the appended k row per element; the V^T column bit-equal to v; every other element of the sentinel-filled K / V^T / Qd
    untouched; a slot outside [0, cap) writes nothing for its sample (the last case: slots 64 and -1 of cap 64)"""
    g = torch.Generator().manual_seed(cap + Hq)
    width, pad = (Hq + 2 * Hkv) * dk, 16
    qkv = torch.randn((B, width + pad), generator=g).bfloat16().to(DEV)
    ang = torch.rand((B, dk // 2), generator=g) * 4000.0
    cos, sin = torch.cos(ang).to(DEV), torch.sin(ang).to(DEV)
    Qd, K, VT = poisoned(B, Hq, dk), poisoned(B, Hkv, cap, dk), poisoned(B, Hkv, dk, cap)
    qd.rope_append(qkv, cos, sin, _i32(slots), Qd, K, VT, B, Hq, Hkv, cap, dk)
    wrote_k, wrote_vt = torch.zeros_like(K, dtype=torch.bool), torch.zeros_like(VT, dtype=torch.bool)
    for b, s in enumerate(slots):
        if not 0 <= s < cap:
            assert bool(is_sentinel(Qd[b]).all())
            continue
        x = qkv[b, :width]
        xq, xk, xv = x[:Hq * dk].view(1, 1, Hq, dk), x[Hq * dk:(Hq + Hkv) * dk].view(1, 1, Hkv, dk), x[(Hq + Hkv) * dk:].view(Hkv, dk)
        QR.check_rope("rope_append q, sample %d" % b, Qd[b].view(1, 1, Hq, dk), xq, cos[b:b + 1, None], sin[b:b + 1, None])
        QR.check_rope("rope_append k, sample %d" % b, K[b, :, s].reshape(1, 1, Hkv, dk), xk, cos[b:b + 1, None], sin[b:b + 1, None])
        assert torch.equal(VT[b, :, :, s], xv)
        wrote_k[b, :, s] = True
        wrote_vt[b, :, :, s] = True
    assert bool(is_sentinel(K)[~wrote_k].all()) and bool(is_sentinel(VT)[~wrote_vt].all())
    assert not bool(is_sentinel(K)[wrote_k].any()) and not bool(is_sentinel(VT)[wrote_vt].any())


# ---------------------------------------------------------------------------------------------------------------- linear
def linear_inputs(B, N, K, seed, rows_w=None):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn((B, K), generator=g).bfloat16().to(DEV)
    W = (torch.randn((rows_w or N, K), generator=g) * K ** -0.5).bfloat16().to(DEV)
    bias = (0.5 * torch.randn((rows_w or N,), generator=g)).bfloat16().to(DEV)
    res = torch.randn((B, N), generator=g).bfloat16().to(DEV)
    return X, W, bias, res


# one wave's k-range partly filled; rows that are no multiple of a workgroup's; eight samples, K no multiple of 512; the 7B's o_proj; its
# down_proj's depth, where the X of two samples is staged in two chunks (the row-0 test below stages eight samples in five)
LINEAR_SHAPES = [(1, 64, 64), (3, 104, 256), (8, 512, 1032), (1, 3584, 3584), (2, 1024, 18944)]


@pytest.mark.parametrize("B,N,K", LINEAR_SHAPES)
@pytest.mark.parametrize("with_bias,with_res", [(False, False), (True, False), (True, True), (False, True)])
def test_decode_linear_vs_fp64_per_element(qd, B, N, K, with_bias, with_res):
    """Row strides wider than the rows everywhere, with sentinels behind the output rows"""
    X, W, bias, res = linear_inputs(B, N, K, seed=N + K)
    Xw, Ww, Rw = poisoned(B, K + 8), poisoned(N, K + 16), poisoned(B, N + 8)
    Xw[:, :K], Ww[:, :K], Rw[:, :N] = X, W, res
    out = poisoned(B, N + 24)
    qd.linear(Xw[:, :K], Ww[:, :K], bias if with_bias else None, Rw[:, :N] if with_res else None, out=out[:, :N])
    want, bound, delta = G.gemm_expect(X, W, bias if with_bias else None, res=res if with_res else None)
    msg, worst, _, _ = G.check_block("decode_linear B=%d N=%d K=%d bias=%s res=%s" % (B, N, K, with_bias, with_res), out[:, :N], want, bound, delta=delta)
    assert msg is None, msg
    print("decode_linear B=%d N=%d K=%d bias=%s res=%s: share of the f32 allowance used %.3f" % (B, N, K, with_bias, with_res, worst))
    assert bool(is_sentinel(out[:, N:]).all())
    # contiguous operands give the same bits
    assert torch.equal(qd.linear(X, W, bias if with_bias else None, res if with_res else None), out[:, :N])


@pytest.mark.parametrize("N,K", [(104, 256), (512, 1032), (64, 18944)])
def test_decode_linear_row_0_is_bit_identical_at_1_and_8_rows(qd, N, K):
    X, W, bias, res = linear_inputs(8, N, K, seed=N)
    y8, y1 = qd.linear(X, W, bias, res), qd.linear(X[:1], W, bias, res[:1])
    assert torch.equal(y8[:1], y1)
    W2, b2 = torch.cat((W, W.flip(0))), torch.cat((bias, bias.flip(0)))
    assert torch.equal(qd.linear(X, W2, b2, gate=True)[:1], qd.linear(X[:1], W2, b2, gate=True))


@pytest.mark.parametrize("B,N,K", [(1, 64, 64), (3, 104, 256), (8, 512, 1032), (1, 9472, 3584), (2, 1024, 1536)])
@pytest.mark.parametrize("with_bias", [False, True])
def test_decode_linear_gate_vs_fp64_per_element(qd, B, N, K, with_bias):
    """mode 1 over the stacked [gate_proj; up_proj] weight: silu(a) b against float64 under qwen_decode_ref.gate_expect's bound"""
    X, W, bias, _ = linear_inputs(B, N, K, seed=N + K + 1, rows_w=2 * N)
    out = poisoned(B, N + 8)
    qd.linear(X, W, bias if with_bias else None, gate=True, out=out[:, :N])
    want, bound, delta = DR.gate_expect(X, W, bias if with_bias else None)
    msg, worst, _, _ = G.check_block("decode_linear gate B=%d N=%d K=%d bias=%s" % (B, N, K, with_bias), out[:, :N], want, bound, delta=delta)
    assert msg is None, msg
    print("decode_linear gate B=%d N=%d K=%d bias=%s: share of the f32 allowance used %.3f" % (B, N, K, with_bias, worst))
    assert bool(is_sentinel(out[:, N:]).all())


def test_decode_linear_refusals(qd):
    from x2i_amd._lib import X2IError
    X, W, bias, res = linear_inputs(2, 64, 64, seed=1)
    out = poisoned(2, 64)
    for bad in (dict(B=0), dict(B=9), dict(ldx=60), dict(ldw=68), dict(ldy=32)):
        with pytest.raises(X2IError):
            qd.linear(X, W, bias, res, out=out, **bad)
    with pytest.raises(X2IError):
        qd.linear(X, torch.cat((W, W)), None, res, out=out, gate=True)           # the gate takes no residual
    assert bool(is_sentinel(out).all())


# ---------------------------------------------------------------------------------------------------------------- the stack
def _library_rows(m, x, mask, pos, dev, dt):
    out = m(inputs_embeds=x.to(device=dev, dtype=dt), attention_mask=None if mask is None else mask.to(dev), position_ids=pos.to(dev),
            output_hidden_states=True, use_cache=False)
    return torch.stack(tuple(out.hidden_states), 1)


T_STEPS = 6
# (hidden, Hq, Hkv, d_ff, layers, B, S, k_lo, k_hi, vl): two configurations of tests/test_qwen_gpu.py's STACK_CASES -- its second (S = 130, four
# heads in two groups) with sample 0 right-padded from 100 and sample 1 left-padded up to 70, and its fourth, Qwen2_5_VLTextModel under three
# differing position axes.  Measured on MI355X over the six decode steps, rel-L2 against float64, HIP / the library's bf16 run on the GPU:
# 3.24e-3 / 4.67e-3 (ratio 0.69), 3.26e-3 / 4.55e-3 (ratio 0.72); the criterion allows 1.5
DECODE_CASES = [(512, 4, 2, 1024, 2, 2, 130, [0, 70], [100, 130], False), (256, 2, 1, 512, 2, 2, 77, None, None, True)]


@pytest.mark.parametrize("hidden,Hq,Hkv,d_ff,layers,B,S,k_lo,k_hi,vl", DECODE_CASES)
def test_prefill_is_forward_and_decode_steps_vs_library_fp64_and_bf16(hidden, Hq, Hkv, d_ff, layers, B, S, k_lo, k_hi, vl):
    from x2i_amd.qwen import Qwen2DecoderStack
    cfg, lib = QR.library_stack(hidden, Hq, Hkv, d_ff, layers, vl=vl)
    sd = QR.random_stack_state_dict(lib, seed=hidden + S)
    lib.load_state_dict(sd, strict=True)
    hip = Qwen2DecoderStack(cfg, device="cpu")
    hip.load_state_dict({k: v.bfloat16() for k, v in sd.items()}, strict=True)
    hip = hip.to(DEV)
    T = T_STEPS
    g = torch.Generator().manual_seed(S)
    x = torch.randn((B, S, hidden), generator=g).bfloat16()
    steps = torch.randn((B, T, hidden), generator=g).bfloat16()
    mask = None
    if k_lo is not None:
        mask = torch.zeros((B, S), dtype=torch.long)
        for b in range(B):
            mask[b, k_lo[b]:k_hi[b]] = 1
    pos = QR.mrope_positions(B, S, seed=S) if vl else torch.arange(S)[None].expand(B, S)
    dev = lambda t: None if t is None else t.to(DEV)
    # prefill: forward's slab bit for bit, and the cache's state
    want = hip(inputs_embeds=dev(x), attention_mask=dev(mask), position_ids=dev(pos)).clone()
    cache = hip.new_cache(B, S + T)
    assert cache.cap == (S + T + 63) // 64 * 64 and cache.K.shape == (layers, B, Hkv, cache.cap, hidden // Hq)
    slab = hip.prefill(cache, inputs_embeds=dev(x), attention_mask=dev(mask), position_ids=dev(pos))
    assert torch.equal(slab, want)
    nxt = DR.next_positions(pos, mask)
    assert cache.k_lo.tolist() == (k_lo or [0] * B) and cache.k_hi.tolist() == (k_hi or [S] * B)
    assert torch.equal(cache.pos.cpu(), nxt.expand_as(cache.pos)) and cache.steps == S
    snap = [t.clone() for t in (cache.K, cache.VT, cache.k_lo, cache.k_hi, cache.pos)]
    # six teacher-forced steps, eager, into the columns of one answer slab
    answer = poisoned(B, layers + 1, T, hidden)
    for t in range(T):
        hip.decode_step(cache, inputs_embeds=dev(steps[:, t:t + 1]), out=answer[:, :, t])
    assert cache.k_hi.tolist() == [h + T for h in (k_hi or [S] * B)] and torch.equal(cache.pos.cpu(), (nxt + T).expand_as(cache.pos))
    assert torch.equal(answer[:, 0], dev(steps)) and cache.steps == S + T
    # ... the same from a restored cache without `out`: bit-identical, and after the first step a step allocates only its output
    def restore():
        for dst, src in zip((cache.K, cache.VT, cache.k_lo, cache.k_hi, cache.pos), snap):
            dst.copy_(src)
        cache.steps = S
    restore()
    xs = dev(steps)
    first = hip.decode_step(cache, inputs_embeds=xs[:, 0:1])
    assert first.shape == (B, layers + 1, 1, hidden) and torch.equal(first[:, :, 0], answer[:, :, 0])
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    second = hip.decode_step(cache, inputs_embeds=xs[:, 1:2])
    assert torch.cuda.memory_stats()["allocation.all.allocated"] - before == 1
    assert torch.equal(second[:, :, 0], answer[:, :, 1])
    # ... and from one captured step replayed six times
    restore()
    static_x = torch.zeros((B, 1, hidden), device=DEV, dtype=torch.bfloat16)
    static_out = torch.zeros((B, layers + 1, hidden), device=DEV, dtype=torch.bfloat16)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                         # (a warm-up step on the capture's stream, then the state put back)
        hip.decode_step(cache, inputs_embeds=static_x, out=static_out)
    torch.cuda.current_stream().wait_stream(side)
    restore()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.decode_step(cache, inputs_embeds=static_x, out=static_out)
    restore()
    replayed = torch.empty_like(answer)
    for t in range(T):
        static_x.copy_(xs[:, t:t + 1])
        graph.replay()
        replayed[:, :, t] = static_out
    assert torch.equal(replayed, answer)
    assert cache.k_hi.tolist() == [h + T for h in (k_hi or [S] * B)]
    # against the library: one full causal pass over prompt + steps under the mask, the steps at the next positions; rows S .. S + T - 1
    xcat = torch.cat((x, steps), 1)
    mcat = None if mask is None else torch.cat((mask, torch.ones((B, T), dtype=torch.long)), 1)
    sp = DR.step_positions(nxt, T)
    pcat = torch.cat((pos, sp.expand(*pos.shape[:-1], T)), -1)
    name = "decode_step hidden=%d %dq/%dkv layers=%d B=%d S=%d range %s..%s vl=%s" % (hidden, Hq, Hkv, layers, B, S, k_lo, k_hi, vl)
    ref = _library_rows(lib.double(), xcat, mcat, pcat, "cpu", torch.float64)[:, :, S:]
    lib_bf16 = _library_rows(lib.to(device=DEV, dtype=torch.bfloat16), xcat, mcat, pcat, DEV, torch.bfloat16)[:, :, S:]
    e_hip, e_lib = QR.rel_l2(answer, ref), QR.rel_l2(lib_bf16, ref)
    print("%s: rel-L2 against float64: HIP %.3e, transformers bf16 on the GPU %.3e (ratio %.2f)" % (name, e_hip, e_lib, e_hip / e_lib))
    assert_stack_criterion(e_hip, e_lib)
    # ... and the float64 restatement of cached decoding (compacted sequences) says the same as the library's padded pass
    rest = DR.decode_reference(sd, x.double(), steps.double(), pos, k_lo, k_hi, num_heads=Hq, num_kv_heads=Hkv, eps=cfg.rms_norm_eps,
                               dk=hidden // Hq, theta=1000000.0, mrope_section=[16, 24, 24] if vl else None)
    assert QR.rel_l2(rest, ref) <= 1e-5           # (the library's float32 norm inside a float64 model: tests/test_qwen_ref_cpu.py)


def test_decode_step_refuses_a_full_or_foreign_cache():
    from x2i_amd.qwen import Qwen2DecoderStack
    kw = dict(hidden_size=256, num_attention_heads=2, num_key_value_heads=1, intermediate_size=512, num_hidden_layers=1, vocab_size=64, device=DEV)
    hip, other = Qwen2DecoderStack(**kw).init_random_(1), Qwen2DecoderStack(**kw)
    cache = hip.new_cache(1, 60)
    ids = torch.randint(0, 64, (1, 62), generator=torch.Generator().manual_seed(3)).to(DEV)
    with pytest.raises(ValueError, match="prefill"):
        hip.decode_step(cache, input_ids=ids[:, :1])
    with pytest.raises(ValueError, match="cap"):
        hip.prefill(cache, input_ids=torch.cat((ids, ids), 1)[:, :64])
    with pytest.raises(ValueError):
        other.prefill(cache, input_ids=ids)
    hip.prefill(cache, input_ids=ids)
    out = hip.decode_step(cache, input_ids=ids[:, :1])
    assert torch.equal(out[:, 0, 0], hip.embed_tokens.weight[ids[:, 0]]) and cache.k_hi.tolist() == [63]
    hip.decode_step(cache, input_ids=ids[:, :1])
    with pytest.raises(ValueError, match="full"):
        hip.decode_step(cache, input_ids=ids[:, :1])


# ---------------------------------------------------------------------------------------------------------------- hand-off
def test_hip_generate_tokens_answer_and_restored_forward():
    """A tiny random Qwen2ForCausalLM (hidden 256, 2 heads of 128, 1 kv head, 3 layers), sample 0 right-padded, 9 new tokens, eager and
    graph-replayed, with a repetition penalty as the logits processor"""
    from transformers import GenerationConfig, Qwen2ForCausalLM
    from transformers.generation.logits_process import RepetitionPenaltyLogitsProcessor
    from x2i_amd.handoff import HipGenerate, HipPrefill, find_decoder
    cfg = QR.library_config(256, 2, 1, 512, 3)
    cfg._attn_implementation = "sdpa"
    torch.manual_seed(0)
    model = Qwen2ForCausalLM(cfg).eval().requires_grad_(False)
    model.model.load_state_dict(QR.random_stack_state_dict(model.model, seed=5), strict=True)
    model = model.to(device=DEV, dtype=torch.bfloat16)
    B, S, T = 2, 77, 9
    ids = torch.randint(0, 64, (B, S), generator=torch.Generator().manual_seed(6)).to(DEV)
    mask = torch.ones((B, S), dtype=torch.long, device=DEV)
    mask[0, 50:] = 0
    logits = model(input_ids=ids, attention_mask=mask, use_cache=False).logits
    hp = HipPrefill(model)
    slab = hp.prefill(model, input_ids=ids, attention_mask=mask).clone()
    hg = HipGenerate(model)
    assert hg.stack.embed_tokens.weight.data_ptr() == model.model.embed_tokens.weight.data_ptr()
    procs = [RepetitionPenaltyLogitsProcessor(1.05)]
    runs = {}
    for graph in (False, True):
        out = runs[graph] = hg.generate(model, max_new_tokens=T, eos_token_id=None, logits_processor=procs, graph=graph, input_ids=ids,
                                        attention_mask=mask)
        assert "forward" not in find_decoder(model).__dict__                                 # the decoder's forward is restored
        assert torch.equal(out.prompt, slab)                                                  # the prompt pass is HipPrefill's
        assert out.answer.shape == (B, 4, T - 1, 256) and out.answer.dtype == torch.bfloat16  # T tokens, T - 1 decode passes
        assert out.sequences.shape == (B, S + T) and torch.equal(out.sequences[:, :S], ids) and out.lengths.tolist() == [T, T]
        # every returned token is the argmax of the model's lm_head (and the processor) over the returned last state before it
        # (token 0 from the last VALID token of each prompt, through the lm_head call of the shape the model itself makes)
        first = model.lm_head(out.prompt[:, -1])[torch.arange(B), torch.tensor([49, S - 1])]
        for t in range(T):
            scores = procs[0](out.sequences[:, :S + t], (first if t == 0 else model.lm_head(out.answer[:, -1, t - 1])).float())
            assert torch.equal(scores.argmax(-1), out.sequences[:, S + t]), t
        # ... and every answer column is the embedding of its token in entry 0
        assert torch.equal(out.answer[:, 0], model.model.embed_tokens.weight[out.sequences[:, S:S + T - 1]])
    assert torch.equal(runs[True].sequences, runs[False].sequences) and torch.equal(runs[True].answer, runs[False].answer)
    # an end token: sample 1's third token ends it; pad follows, the lengths say so, and the host's look every 2 steps stops the loop early
    seq = runs[False].sequences
    eos = int(seq[1, S + 2])
    stop0 = [t for t in range(T) if int(seq[0, S + t]) == eos]
    out = hg.generate(model, max_new_tokens=T, eos_token_id=eos, pad_token_id=63, logits_processor=procs, graph=False, check_every=2, input_ids=ids,
                      attention_mask=mask)
    n1 = min(t for t in range(T) if int(seq[1, S + t]) == eos) + 1
    n0 = stop0[0] + 1 if stop0 else T
    n = max(n0, n1)
    assert out.lengths.tolist() == [n0, n1] and out.sequences.shape == (B, S + n) and out.answer.shape[2] == n - 1
    assert torch.equal(out.sequences[1, S:S + n1], seq[1, S:S + n1]) and bool((out.sequences[1, S + n1:] == 63).all())
    assert torch.equal(out.sequences[0, S:S + n0], seq[0, S:S + n0])
    # afterwards HipPrefill and a plain library call give what they gave before
    assert torch.equal(model(input_ids=ids, attention_mask=mask, use_cache=False).logits, logits)
    assert torch.equal(hp.prefill(model, input_ids=ids, attention_mask=mask), slab)
    # a generation_config that samples is refused by name, before anything runs; the forward stays the model's own
    with pytest.raises(ValueError, match="--full_generate"):
        hg.generate(model, max_new_tokens=T, generation_config=GenerationConfig(do_sample=True, top_k=50), input_ids=ids, attention_mask=mask)
    assert "forward" not in find_decoder(model).__dict__
    # ... and after an exception inside the prompt pass too
    with pytest.raises(ValueError, match="contiguous"):
        hole = mask.clone()
        hole[1, 10] = 0
        hg.generate(model, max_new_tokens=T, input_ids=ids, attention_mask=hole)
    assert "forward" not in find_decoder(model).__dict__
