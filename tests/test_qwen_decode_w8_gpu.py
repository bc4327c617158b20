"""GPU checks of the e4m3 weight-only decode steps (include/x2i_qwen_decode_w8.h, Qwen2DecoderStack.pack_w8 / decode_step(w8=True),
handoff.HipGenerate(w8=True)): every e4m3 code exactly, the entry point per element against float64 over the dequantised weight
(tests/qwen_decode_w8_ref.py) with poisoned surroundings, its two bit-level promises, its refusals, the stack against the float64 restatement
of the QUANTISED model, the hand-off's four loops, and the drift against the bf16 weights (recorded, on random weights).

The figures measured on the MI355X stand in the docstrings of the tests and in DESIGN.md section 4, "e4m3 weight-only decode"."""
import pytest
import torch

from tests import fp8_ref as F8
from tests import gemm_ref as G
from tests import qwen_decode_ref as DR
from tests import qwen_decode_w8_ref as WR
from tests import qwen_ref as QR
from tests.test_qwen_decode_w8_ref_cpu import w8_inputs
from tests.test_t5_gpu import assert_stack_criterion, is_sentinel, poisoned  # (helpers; its tests are not re-collected here)

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def w8():
    from x2i_amd import qwen_decode_w8_ops as o
    o.load()
    return o


def dev(*ts):
    return tuple(None if t is None else t.to(DEV) for t in ts)


# ---------------------------------------------------------------------------------------------------------------- every code
def test_every_e4m3_code_decodes_exactly(w8):
    """K = 256, N = 16: row n holds the codes 0 .. 255 rotated by 16 n (0x7F and 0xFF, NaN, replaced by 0), X is one-hot, eight rows per
    launch, 32 launches: every output is bf16(f32(scale[n] * e4m3(code))) bit for bit, with scales that are no powers of two.  (The sum
    starts at +0, so the code 0x80, -0, gives +0: the expectation adds +0 as the kernel does.)"""
    K, N = 256, 16
    codes = ((torch.arange(K)[None] + 16 * torch.arange(N)[:, None]) % 256).to(torch.uint8)
    codes[(codes & 0x7F) == 0x7F] = 0
    scale = (0.0123456789 * (1.0 + torch.arange(N) / 7.0)).float()
    val = F8.decode(codes).float()                                     # [N, K], exact
    want = ((scale[:, None] * val + 0.0).T.contiguous()).bfloat16()    # [K, N]: row k is the output of the one-hot at k
    W8d, sd = dev(codes, scale)
    got = torch.empty((K, N), dtype=torch.bfloat16, device=DEV)
    eye = torch.eye(K, dtype=torch.bfloat16, device=DEV)
    for k0 in range(0, K, 8):
        w8.linear_w8(eye[k0:k0 + 8], W8d, sd, out=got[k0:k0 + 8])
    bad = got.cpu().view(torch.int16) != want.view(torch.int16)
    assert not bool(bad.any()), "codes decoded wrongly (k, n): %s" % bad.nonzero()[:8].tolist()
    # ... and the torch.float8_e4m3fn view of the same codes is accepted and gives the same bits
    assert torch.equal(w8.linear_w8(eye[:8], W8d.view(torch.float8_e4m3fn), sd), got[:8])


# ---------------------------------------------------------------------------------------------------------------- per element
def wide_operands(X, W8, res, B, N, K):
    """X, W8 and res inside poisoned buffers whose rows are wider than theirs (the weight's padding holds the NaN code 0x7F)"""
    Xw, Rw = poisoned(B, K + 8), poisoned(B, N + 8)
    Ww = torch.full((W8.shape[0], K + 32), 0x7F, dtype=torch.uint8, device=DEV)
    Xw[:, :K], Ww[:, :K], Rw[:, :N] = X.to(DEV), W8.to(DEV), res.to(DEV)
    return Xw[:, :K], Ww[:, :K], Rw[:, :N]


# four lanes of a wave hold data; N no multiple of a workgroup's rows and lane 17 the last; the second k-step has one lane; X staged in two
# chunks, the second of 16 columns; the model's own width
LINEAR_SHAPES = [(1, 64, 64), (3, 104, 272), (8, 512, 1040), (8, 64, 4112), (1, 3584, 3584)]


@pytest.mark.parametrize("B,N,K", LINEAR_SHAPES)
@pytest.mark.parametrize("with_bias,with_res", [(False, False), (True, False), (True, True), (False, True)])
def test_linear_w8_vs_fp64_per_element(w8, B, N, K, with_bias, with_res):
    """Measured on the MI355X: 0.000 of the f32 allowance used in each of the twenty cases (no error beyond the output's one rounding)"""
    X, W8, s, bias, res = w8_inputs(B, N, K, seed=N + K)
    Xv, Wv, Rv = wide_operands(X, W8, res, B, N, K)
    out = poisoned(B, N + 24)
    sd, bd = dev(s, bias)
    w8.linear_w8(Xv, Wv, sd, bd if with_bias else None, Rv if with_res else None, out=out[:, :N])
    want, bound, delta = WR.linear_w8_expect(X, W8, s, bias if with_bias else None, res if with_res else None)
    name = "decode_linear_w8 B=%d N=%d K=%d bias=%s res=%s" % (B, N, K, with_bias, with_res)
    msg, worst, _, _ = G.check_block(name, out[:, :N].cpu(), want, bound, delta=delta)
    print("%s: share of the f32 allowance used %.3f" % (name, worst))
    assert msg is None, msg
    assert bool(is_sentinel(out[:, N:]).all())
    # contiguous operands give the same bits, and Y may be res
    Xd, Wd, Rd = dev(X, W8, res)
    assert torch.equal(w8.linear_w8(Xd, Wd, sd, bd if with_bias else None, Rd if with_res else None), out[:, :N])
    if with_res:
        w8.linear_w8(Xd, Wd, sd, bd if with_bias else None, Rd, out=Rd)
        assert torch.equal(Rd, out[:, :N])


@pytest.mark.parametrize("B,N,K", [(1, 64, 64), (3, 104, 272), (8, 512, 1040), (2, 1024, 1536)])
@pytest.mark.parametrize("with_bias", [False, True])
def test_linear_w8_gate_vs_fp64_per_element(w8, B, N, K, with_bias):
    """mode 1 over the stacked weight whose `b` rows carry scales at least 4 times the `a` rows': a wrong scale index cannot hide.
    Measured on the MI355X: 0.000 of the f32 allowance used in each of the eight cases"""
    X, W8, s, bias, res = w8_inputs(B, N, K, seed=N + K + 1, rows_w=2 * N, split_scales=True)
    assert float((s[N:] / s[:N]).min()) >= 4.0
    Xv, Wv, _ = wide_operands(X, W8, res, B, N, K)
    out = poisoned(B, N + 8)
    sd, bd = dev(s, bias)
    w8.linear_w8(Xv, Wv, sd, bd if with_bias else None, gate=True, out=out[:, :N])
    want, bound, delta = WR.gate_w8_expect(X, W8, s, bias if with_bias else None)
    name = "decode_linear_w8 gate B=%d N=%d K=%d bias=%s" % (B, N, K, with_bias)
    msg, worst, _, _ = G.check_block(name, out[:, :N].cpu(), want, bound, delta=delta)
    print("%s: share of the f32 allowance used %.3f" % (name, worst))
    assert msg is None, msg
    assert bool(is_sentinel(out[:, N:]).all())


# ---------------------------------------------------------------------------------------------------------------- the two promises
@pytest.mark.parametrize("N,K", [(104, 272), (512, 1040), (64, 4112)])
def test_linear_w8_row_0_is_bit_identical_at_1_and_8_rows_and_on_a_relaunch(w8, N, K):
    """(64, 4112): X unchunked at B = 1, staged in two chunks at B = 8"""
    X, W8, s, bias, res = dev(*w8_inputs(8, N, K, seed=N))
    y8, y1 = w8.linear_w8(X, W8, s, bias, res), w8.linear_w8(X[:1], W8, s, bias, res[:1])
    assert torch.equal(y8[:1], y1)
    assert torch.equal(w8.linear_w8(X, W8, s, bias, res), y8)
    W2, s2, b2 = torch.cat((W8, W8.flip(0))), torch.cat((s, 4.0 * s.flip(0))), torch.cat((bias, bias.flip(0)))
    g8, g1 = w8.linear_w8(X, W2, s2, b2, gate=True), w8.linear_w8(X[:1], W2, s2, b2, gate=True)
    assert torch.equal(g8[:1], g1)
    assert torch.equal(w8.linear_w8(X, W2, s2, b2, gate=True), g8)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_linear_w8_refusals_launch_nothing(w8):
    from x2i_amd._lib import X2IError
    X, W8, s, bias, res = dev(*w8_inputs(2, 64, 64, seed=1))
    out = poisoned(2, 64)
    X72 = torch.zeros((2, 72), dtype=torch.bfloat16, device=DEV)
    W72 = torch.zeros((64, 80), dtype=torch.uint8, device=DEV)
    odd = torch.zeros((64 * 64 + 16,), dtype=torch.uint8, device=DEV)[8:8 + 64 * 64].view(64, 64)       # 8 bytes off a 16-byte boundary
    assert odd.data_ptr() % 16 == 8
    cases = [lambda: w8.linear_w8(X72, W72[:, :72], s, bias, res, out=out),                 # K % 16 != 0
             lambda: w8.linear_w8(X, W8, s, bias, res, out=out, B=0), lambda: w8.linear_w8(X, W8, s, bias, res, out=out, B=9),
             lambda: w8.linear_w8(X, torch.cat((W8, W8)), torch.cat((s, s)), None, res, out=out, gate=True),      # res in mode 1
             lambda: w8.linear_w8(X, odd, s, bias, res, out=out),                            # misaligned W8
             lambda: w8.linear_w8(X, W8, s, bias, res, out=out, ldw=48)]                     # ldw < K
    for i, f in enumerate(cases):
        with pytest.raises(X2IError):
            f()
        assert bool(is_sentinel(out).all()), i
    # a NULL scale: straight at the entry point (the binding never passes one)
    from x2i_amd import ops
    rc = w8.load().x2i_qwen_decode_linear_w8_bf16(ops._p(X), 64, ops._p(W8), 64, None, None, None, 0, ops._p(out), 64, 2, 64, 64, 0, ops._stream())
    assert rc == -1 and b"w_scale" in w8.load().x2i_last_error()
    torch.cuda.synchronize()
    assert bool(is_sentinel(out).all())
    with pytest.raises(X2IError):
        w8.linear_w8(X, W8.view(torch.int8), s)                                              # neither e4m3 nor uint8


# ---------------------------------------------------------------------------------------------------------------- the stack
T_STEPS = 6
# (hidden, Hq, Hkv, d_ff, layers, B, S, k_lo, k_hi, vl): tests/test_qwen_decode_gpu.py's DECODE_CASES, restated
DECODE_CASES = [(512, 4, 2, 1024, 2, 2, 130, [0, 70], [100, 130], False), (256, 2, 1, 512, 2, 2, 77, None, None, True)]


def _library_rows(m, x, mask, pos, d, dt):
    out = m(inputs_embeds=x.to(device=d, dtype=dt), attention_mask=None if mask is None else mask.to(d), position_ids=pos.to(d),
            output_hidden_states=True, use_cache=False)
    return torch.stack(tuple(out.hidden_states), 1)


@pytest.mark.parametrize("hidden,Hq,Hkv,d_ff,layers,B,S,k_lo,k_hi,vl", DECODE_CASES)
def test_w8_decode_steps_vs_fp64_of_the_quantised_model(hidden, Hq, Hkv, d_ff, layers, B, S, k_lo, k_hi, vl):
    """The quantised model is the model under test: the reference is the float64 restatement of cached decoding with the seven projections
    per layer replaced by their dequantised float64 values FOR THE STEP TOKENS (qwen_decode_w8_ref.decode_reference_w8).  The prompt
    tokens run on the bf16 weights there as they do here -- prefill is untouched and fills the cache the steps attend to; with the
    dequantised weights over the prompt too the reference describes another model, and the steps measure 8.8e-3 / 9.3e-3 against it, the
    format's drift of the prompt's keys and values (printed below).  The bound is the one tests/test_qwen_decode_gpu.py holds the bf16
    step to: at most 1.5 times the error of the library's bf16 run on the GPU against ITS float64 reference, and under 3e-2.
    Measured on the MI355X, rel-L2 against float64, w8 steps / bf16 steps / the library's bf16 run: 3.27e-3 / 3.24e-3 / 4.67e-3 (ratio
    0.70) and 3.28e-3 / 3.26e-3 / 4.55e-3 (ratio 0.72)."""
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
    xd, md, pd, sdv = dev(x, mask, pos, steps)

    def run(w8):
        cache = hip.new_cache(B, S + T)
        slab = hip.prefill(cache, inputs_embeds=xd, attention_mask=md, position_ids=pd).clone()
        answer = poisoned(B, layers + 1, T, hidden)
        for t in range(T):
            hip.decode_step(cache, inputs_embeds=sdv[:, t:t + 1], out=answer[:, :, t], w8=w8)
        return slab, answer

    with pytest.raises(ValueError, match="pack_w8"):
        hip.decode_step(hip.new_cache(B, S + T), inputs_embeds=sdv[:, :1], w8=True)          # (refused before the cache is looked at)
    slab0, bf16 = run(False)
    assert hip.pack_w8() is hip and len(hip._w8) == layers
    for nm, (codes, scale) in hip._w8[0].items():
        assert codes.dtype == torch.float8_e4m3fn and scale.dtype == torch.float32 and scale.shape == (codes.shape[0],), nm
    slab1, again = run(False)
    assert torch.equal(slab1, slab0)                       # the prefill slab with a pack present
    assert torch.equal(again, bf16)                        # decode_step(w8=False) after pack_w8(): the parent's bits
    slab2, answer = run(True)
    assert torch.equal(slab2, slab0) and torch.equal(answer[:, 0], sdv) and not torch.equal(answer, bf16)
    # the pack is what the CPU quantiser says, bit for bit (so the float64 reference below is of exactly these weights)
    c_ref, s_ref = WR.quantize_rows(sd["layers.0.mlp.down_proj.weight"].bfloat16())
    assert torch.equal(hip._w8[0]["down"][0].view(torch.uint8).cpu(), c_ref) and torch.equal(hip._w8[0]["down"][1].cpu(), s_ref)
    name = "w8 decode_step hidden=%d %dq/%dkv layers=%d B=%d S=%d range %s..%s vl=%s" % (hidden, Hq, Hkv, layers, B, S, k_lo, k_hi, vl)
    kw = dict(num_heads=Hq, num_kv_heads=Hkv, eps=cfg.rms_norm_eps, dk=hidden // Hq, theta=1000000.0, mrope_section=[16, 24, 24] if vl else None)
    ref8 = WR.decode_reference_w8(sd, x.double(), steps.double(), pos, k_lo, k_hi, **kw)
    all8 = DR.decode_reference(WR.dequantized_state_dict(sd, Hq, Hkv), x.double(), steps.double(), pos, k_lo, k_hi, **kw)
    # the yardstick: the library in bf16 on the GPU against the library in float64, both on the bf16 weights (the parent test's e_lib)
    xcat = torch.cat((x, steps), 1)
    mcat = None if mask is None else torch.cat((mask, torch.ones((B, T), dtype=torch.long)), 1)
    nxt = DR.next_positions(pos, mask)
    pcat = torch.cat((pos, DR.step_positions(nxt, T).expand(*pos.shape[:-1], T)), -1)
    ref = _library_rows(lib.double(), xcat, mcat, pcat, "cpu", torch.float64)[:, :, S:]
    lib_bf16 = _library_rows(lib.to(device=DEV, dtype=torch.bfloat16), xcat, mcat, pcat, DEV, torch.bfloat16)[:, :, S:]
    e_hip, e_lib, e_bf = QR.rel_l2(answer, ref8), QR.rel_l2(lib_bf16, ref), QR.rel_l2(bf16, ref)
    print("%s: rel-L2 against float64: w8 steps (quantised model) %.3e, bf16 steps (bf16 model) %.3e, transformers bf16 on the GPU %.3e (ratio %.2f); "
          "w8 steps against the model quantised over the prompt too %.3e" % (name, e_hip, e_bf, e_lib, e_hip / e_lib, QR.rel_l2(answer, all8)))
    assert_stack_criterion(e_hip, e_lib)


def test_pack_w8_zero_rows_are_finite_and_the_pack_goes_stale_with_the_weights():
    from x2i_amd.qwen import Qwen2DecoderStack
    kw = dict(hidden_size=256, num_attention_heads=2, num_key_value_heads=1, intermediate_size=512, num_hidden_layers=2, vocab_size=64, device=DEV)
    hip = Qwen2DecoderStack(**kw).init_random_(1)
    with torch.no_grad():                                   # all-zero output rows in each of the four weights of layer 0
        hip._fused["0.qkv.w"][3].zero_()
        hip._fused["0.gu"][5].zero_()
        hip._fused["0.gu"][512 + 9].zero_()
        hip.layers[0].self_attn.o_proj.weight[7].zero_()
        hip.layers[0].mlp.down_proj.weight[11].zero_()
    hip.pack_w8()
    for nm, row in (("qkv", 3), ("gu", 5), ("gu", 521), ("o", 7), ("down", 11)):
        codes, scale = hip._w8[0][nm]
        assert float(scale[row]) == 1.0 and bool((codes[row].view(torch.uint8) == 0).all()), nm
    ids = torch.randint(0, 64, (1, 20), generator=torch.Generator().manual_seed(3)).to(DEV)
    cache = hip.new_cache(1, 24)
    hip.prefill(cache, input_ids=ids)
    out = hip.decode_step(cache, input_ids=ids[:, :1], w8=True)
    assert bool(torch.isfinite(out.float()).all())
    # ... and a zero row gives exactly its bias: row 3 of layer 0's q|k|v through the entry point
    from x2i_amd.qwen_decode_w8_ops import linear_w8
    y = linear_w8(cache.NRM, *hip._w8[0]["qkv"], hip._fused["0.qkv.b"])
    assert torch.equal(y[:, 3], hip._fused["0.qkv.b"][3].expand(1))
    # load_state_dict, .to() and init_random_ drop the pack; w8=True then raises until the stack is repacked
    pack = hip._w8
    hip.load_state_dict(hip.state_dict())
    assert hip._w8 is None
    with pytest.raises(ValueError, match="pack_w8"):
        hip.decode_step(cache, input_ids=ids[:, :1], w8=True)
    hip.pack_w8()
    assert hip._w8 is not pack and torch.equal(hip._w8[1]["o"][0].view(torch.uint8), pack[1]["o"][0].view(torch.uint8))
    again = hip.decode_step(cache, input_ids=ids[:, :1], w8=True)
    assert bool(torch.isfinite(again.float()).all())
    hip.init_random_(2)
    assert hip._w8 is None
    hip.pack_w8()
    hip.to(DEV)
    assert hip._w8 is None


# ---------------------------------------------------------------------------------------------------------------- hand-off
def _tiny_model():
    from transformers import Qwen2ForCausalLM
    cfg = QR.library_config(256, 2, 1, 512, 3)
    cfg._attn_implementation = "sdpa"
    torch.manual_seed(0)
    model = Qwen2ForCausalLM(cfg).eval().requires_grad_(False)
    model.model.load_state_dict(QR.random_stack_state_dict(model.model, seed=5), strict=True)
    return model.to(device=DEV, dtype=torch.bfloat16)


@pytest.mark.parametrize("hip_head", [False, True])
def test_hip_generate_w8_graph_equals_eager_and_the_option_switches_cleanly(hip_head):
    """tests/test_qwen_decode_gpu.py's tiny Qwen2ForCausalLM, sample 0 right-padded, 9 new tokens, under the torch head and the HIP head:
    bf16 first (the parent's loop), then w8 eager and graph-replayed, then bf16 again -- which must not replay the w8 graph"""
    from transformers.generation.logits_process import RepetitionPenaltyLogitsProcessor
    from x2i_amd.handoff import HipGenerate, find_decoder
    model = _tiny_model()
    B, S, T = 2, 77, 9
    ids = torch.randint(0, 64, (B, S), generator=torch.Generator().manual_seed(6)).to(DEV)
    mask = torch.ones((B, S), dtype=torch.long, device=DEV)
    mask[0, 50:] = 0
    procs = [RepetitionPenaltyLogitsProcessor(1.05)]
    hg = HipGenerate(model, hip_head=hip_head)
    gen = lambda **kw: hg.generate(model, max_new_tokens=T, eos_token_id=None, logits_processor=procs, input_ids=ids, attention_mask=mask, **kw)
    base = gen(graph=True)
    assert hg.stack._w8 is None                                                              # no pack until the option asks for one
    runs = {}
    for graph in (False, True, True):                                                        # (the third: a replay of the kept w8 graph)
        out = gen(graph=graph, w8=True)
        runs.setdefault(graph, out)
        assert "forward" not in find_decoder(model).__dict__                                 # the decoder's forward is restored
        assert torch.equal(out.prompt, base.prompt)                                           # the prompt pass stays bf16
        assert out.answer.shape == (B, 4, T - 1, 256) and out.sequences.shape == (B, S + T) and out.lengths.tolist() == [T, T]
        assert torch.equal(out.answer[:, 0], model.model.embed_tokens.weight[out.sequences[:, S:S + T - 1]])
        assert torch.equal(out.sequences, runs[False].sequences) and torch.equal(out.answer, runs[False].answer)     # graph == eager
    assert hg.stack._w8 is not None
    assert not torch.equal(runs[True].answer[:, 1:, 0], base.answer[:, 1:, 0])               # the w8 steps are other arithmetic
    after = gen(graph=True)                                                                   # w8=False after w8=True: the parent's bits
    assert torch.equal(after.sequences, base.sequences) and torch.equal(after.answer, base.answer)
    eager = gen(graph=False)
    assert torch.equal(eager.sequences, base.sequences) and torch.equal(eager.answer, base.answer)
    # the constructor's default, overridden per call
    hg.w8 = True
    assert torch.equal(gen(graph=True).answer, runs[True].answer) and torch.equal(gen(graph=True, w8=False).answer, base.answer)


# ---------------------------------------------------------------------------------------------------------------- drift
@pytest.mark.parametrize("seed", [11, 12, 13])
def test_w8_drift_against_the_bf16_weights_is_the_formats_own(seed):
    """Recorded, not asserted against an invented number: the rel-L2 of the answer slab of the w8 steps against the bf16 steps on identical
    token ids, beside the same quantity in float64 on the CPU from the two state dicts (the format's own drift, from the reference).  Each
    GPU form lies within the parent test's step bound (3e-2, assert_stack_criterion) of its float64 reference, so the two drifts may
    differ by that much and no more.  Random weights: real checkpoints are not measured here.
    Measured on the MI355X (GPU / float64): 2.95e-2 / 2.91e-2, 3.10e-2 / 3.03e-2, 3.04e-2 / 2.99e-2."""
    from x2i_amd.qwen import Qwen2DecoderStack
    hidden, Hq, Hkv, d_ff, layers, B, S, T = 256, 2, 1, 512, 2, 2, 40, 6
    cfg, lib = QR.library_stack(hidden, Hq, Hkv, d_ff, layers)
    sd = QR.random_stack_state_dict(lib, seed=seed)
    hip = Qwen2DecoderStack(cfg, device="cpu")
    hip.load_state_dict({k: v.bfloat16() for k, v in sd.items()}, strict=True)
    hip = hip.to(DEV).pack_w8()
    g = torch.Generator().manual_seed(seed)
    ids, step_ids = torch.randint(0, 64, (B, S), generator=g), torch.randint(0, 64, (B, T), generator=g)
    out = {}
    for w8 in (False, True):
        cache = hip.new_cache(B, S + T)
        hip.prefill(cache, input_ids=ids.to(DEV))
        out[w8] = torch.empty((B, layers + 1, T, hidden), dtype=torch.bfloat16, device=DEV)
        for t in range(T):
            hip.decode_step(cache, input_ids=step_ids[:, t].to(DEV), out=out[w8][:, :, t], w8=w8)
    table = sd["embed_tokens.weight"].double()
    pos = torch.arange(S)[None].expand(B, S)
    kw = dict(num_heads=Hq, num_kv_heads=Hkv, eps=cfg.rms_norm_eps, dk=hidden // Hq, theta=1000000.0)
    r16 = DR.decode_reference(sd, table[ids], table[step_ids], pos, None, None, **kw)
    r8 = WR.decode_reference_w8(sd, table[ids], table[step_ids], pos, None, None, **kw)       # (the prompt on the bf16 weights, as on the GPU)
    # entry 0 (the embeddings) is common to both: the drift is over the layers' outputs
    d_gpu, d_f64 = QR.rel_l2(out[True][:, 1:], out[False][:, 1:].double().cpu()), QR.rel_l2(r8[:, 1:], r16[:, 1:])
    print("w8 drift, seed %d, random weights: answer slab rel-L2 w8 against bf16 weights: GPU %.3e, float64 reference %.3e" % (seed, d_gpu, d_f64))
    assert abs(d_gpu - d_f64) <= 3e-2
