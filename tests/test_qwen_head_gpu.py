"""Token selection on the HIP path (GPU): the two kernels of include/x2i_qwen_head.h against the float64 reference tests/qwen_head_ref.py --
logits per element, independence of row position and batch, the choice of the token with planted winners and ties, the penalty's bits against
the library's processor, the bookkeeping -- and HipGenerate(hip_head=True) and the multi-turn conditioner on a tiny Qwen2ForCausalLM."""
import pytest
import torch

from tests import gemm_ref as G
from tests import qwen_head_ref as HR
from tests import qwen_ref as QR

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEEN_SENTINEL = 0x5A


@pytest.fixture(scope="module")
def ho():
    from x2i_amd import qwen_head_ops
    qwen_head_ops.load()
    return qwen_head_ops


def head_inputs(B, V, K, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn((B, K), generator=g).bfloat16().to(DEV)
    W = (torch.randn((V, K), generator=g) * K ** -0.5).bfloat16().to(DEV)
    return X, W


def plant(W, X, b, n, c):
    """add c to sample b's logit of row n: a multiple of X's own row onto W's"""
    x = X[b].float()
    W[n] = (W[n].float() + c * x / float(x.pow(2).sum())).bfloat16()


class State:
    """the device state of one generation loop, with sentinels around what select may write"""

    def __init__(self, B, V, ncols, col, eos=(), seen=True, done=None):
        self.B, self.V, self.ncols = B, V, ncols
        self.step = torch.tensor([col], device=DEV, dtype=torch.int32)
        self.token = torch.full((B,), -7, device=DEV, dtype=torch.long)
        self.seq_buf = torch.full((B, ncols + 3), -7, device=DEV, dtype=torch.long)
        self.seq = self.seq_buf[:, :ncols]
        self.lengths = torch.zeros((B,), device=DEV, dtype=torch.long)
        self.done = torch.tensor(done if done is not None else [0] * B, device=DEV, dtype=torch.uint8)
        self.eos = torch.tensor(list(eos), device=DEV, dtype=torch.long) if eos else None
        self.seen_buf = torch.zeros((B, V + 5), device=DEV, dtype=torch.uint8) if seen else None
        self.seen = self.seen_buf[:, :V] if seen else None

    def snapshot(self):
        c = lambda t: None if t is None else t.clone()
        return dict(step=c(self.step), token=c(self.token), seq=c(self.seq_buf), lengths=c(self.lengths), done=c(self.done), seen=c(self.seen_buf))


def run(ho, X, W, st, penalty=1.0, pad=0, logits=None, ws=None):
    B, V = X.shape[0], W.shape[0]
    ws = torch.empty((ho.workspace_floats(B, V),), device=DEV, dtype=torch.float32) if ws is None else ws
    ho.logits_argmax(X, W, ws, seen=st.seen, penalty=penalty, logits=logits, step=st.step)
    ho.select(ws, st.step, st.token, st.seq, st.lengths, st.done, pad, V, eos=st.eos, seen=st.seen)
    return st.token.clone()


def run_logits(ho, X, W, seen=None, penalty=1.0, padded=True):
    """-> (logits [B, V] view, its sentinel-filled buffer): padded ldx / ldw / ldl / ld_seen"""
    B, K = X.shape
    V = W.shape[0]
    if padded:
        Xw, Ww = torch.zeros((B, K + 8), device=DEV, dtype=torch.bfloat16), torch.zeros((V, K + 16), device=DEV, dtype=torch.bfloat16)
        G.poison_(Xw), G.poison_(Ww)
        Xw[:, :K], Ww[:, :K] = X, W
        X, W = Xw[:, :K], Ww[:, :K]
        if seen is not None:
            sw = torch.full((B, V + 3), 1, device=DEV, dtype=torch.uint8)
            sw[:, :V] = seen
            seen = sw[:, :V]
    buf = G.poison_(torch.empty((B, V + 8), device=DEV, dtype=torch.float32))
    ws = torch.empty((ho.workspace_floats(B, V),), device=DEV, dtype=torch.float32)
    ho.logits_argmax(X, W, ws, seen=seen, penalty=penalty, logits=buf[:, :V])
    return buf[:, :V], buf


# ---------------------------------------------------------------------------------------------------------------- logits
# one wave's k-range partly filled; V no multiple of a workgroup's rows; eight samples, a prime V, K no multiple of 512; the models' K; the real
# vocabulary's workgroup count
LOGIT_SHAPES = [(1, 64, 64), (3, 1000, 256), (8, 4099, 1032), (1, 2048, 3584), (2, 2048, 2048), (1, 152064, 64)]


@pytest.mark.parametrize("B,V,K", LOGIT_SHAPES)
def test_logits_vs_fp64_per_element(ho, B, V, K):
    X, W = head_inputs(B, V, K, seed=V + K)
    seen = (torch.rand((B, V), generator=torch.Generator().manual_seed(V)) < 0.3).to(torch.uint8).to(DEV)
    for s, pen in ((None, 1.0), (seen, 1.3)):
        out, buf = run_logits(ho, X, W, s, pen)
        want, bound, delta = HR.head_expect(X, W, s, pen)
        msg, worst, _, _ = G.check_block("head logits B=%d V=%d K=%d penalty=%s" % (B, V, K, pen), out, want, bound, delta=delta)
        assert msg is None, msg
        print("head logits B=%d V=%d K=%d penalty=%s: share of the f32 allowance used %.3f" % (B, V, K, pen, worst))
        assert bool(G.sentinel_bits(buf[:, V:]).all())                      # nothing outside the V columns
        # contiguous operands give the same bits
        assert torch.equal(run_logits(ho, X, W, s, pen, padded=False)[0], out)


def test_logits_with_x_staged_in_chunks_and_the_bits_of_decode_linear(ho):
    """B * K bf16 past what one workgroup stages at once (two column chunks); and a logit is decode_linear's mode-0 sum bit for bit: rounded
    to bf16 it is that kernel's output"""
    from x2i_amd import qwen_decode_ops as qd
    for B, V, K in ((8, 64, 4104), (3, 1000, 256)):
        X, W = head_inputs(B, V, K, seed=K)
        out, buf = run_logits(ho, X, W)
        want, bound, delta = HR.head_expect(X, W)
        msg, worst, _, _ = G.check_block("head logits B=%d V=%d K=%d" % (B, V, K), out, want, bound, delta=delta)
        assert msg is None, msg
        print("head logits B=%d V=%d K=%d: share of the f32 allowance used %.3f" % (B, V, K, worst))
        assert bool(G.sentinel_bits(buf[:, V:]).all())
        assert torch.equal(G.bf16_rne(out.double()).bfloat16(), qd.linear(X, W))


def test_logits_do_not_depend_on_batch_row_position_or_launch(ho):
    B, V, K = 8, 4099, 1032
    X, W = head_inputs(B, V, K, seed=11)
    tail = (V // ho.ROWS) * ho.ROWS                                          # the first row of the last, partly filled workgroup
    for n in (0, V // 2, tail, V - 1):
        W[n] = W[7]
    l8, _ = run_logits(ho, X, W)
    l1, _ = run_logits(ho, X[:1], W)
    assert torch.equal(l8[:1], l1)                                          # row 0 at B = 1 and B = 8
    assert torch.equal(run_logits(ho, X, W)[0], l8)                         # a relaunch
    for n in (0, V // 2, tail, V - 1):
        assert torch.equal(l8[:, n], l8[:, 7]), n                           # one W row wherever it falls in a wave or workgroup
    # ... and not on V: the first 1000 rows alone
    assert torch.equal(run_logits(ho, X, W[:1000])[0], l8[:, :1000])


def test_penalty_bits_are_the_librarys_processor_in_f32(ho):
    from transformers.generation.logits_process import RepetitionPenaltyLogitsProcessor
    B, V, K = 3, 1000, 256
    X, W = head_inputs(B, V, K, seed=5)
    ids = torch.randint(0, V, (B, 300), generator=torch.Generator().manual_seed(6)).to(DEV)
    plain, _ = run_logits(ho, X, W)
    got, _ = run_logits(ho, X, W, HR.seen_of(ids, V), 1.05)
    # (the processor on the CPU: there torch's `score / penalty` is the true division of the contract; its GPU kernel multiplies by 1 / penalty)
    want = RepetitionPenaltyLogitsProcessor(1.05)(ids.cpu(), plain.cpu().clone())
    assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))
    assert int((got != plain).sum()) > 200 and bool((plain < 0).any()) and bool((plain > 0).any())


# ---------------------------------------------------------------------------------------------------------------- selection
def assert_determined(want, bound, what, equals=()):
    gap, allow = HR.margin(want, bound, equals=equals)
    assert bool((gap > allow).all()), "%s: the float64 margin %s does not exceed twice the bound %s: the inputs do not determine a token" % (
        what, gap.tolist(), allow.tolist())


@pytest.mark.parametrize("B,V,K,winners", [(1, 1000, 256, [0]), (1, 1000, 256, [999]), (2, 1000, 256, [993, 992]),
                                           (8, 4099, 1032, [0, 4098, 4097, 2049, 17, 4096, 16, 1023]), (1, 152064, 64, [152063])])
def test_select_finds_planted_winners(ho, B, V, K, winners):
    X, W = head_inputs(B, V, K, seed=V + K + 1)
    for b, n in enumerate(winners):
        plant(W, X, b, n, 9.0)
    want, bound, _ = HR.head_expect(X, W)
    assert_determined(want, bound, "planted winners %s" % winners)
    assert HR.argmax_lowest(want).tolist() == winners
    st = State(B, V, 4, 1)
    assert run(ho, X, W, st).tolist() == winners


def test_select_ties_take_the_lowest_index_and_the_penalty_moves_them(ho):
    B, V, K = 2, 4099, 256
    X, W = head_inputs(B, V, K, seed=21)
    X[1] = X[0]
    plant(W, X, 0, 70, 9.0)
    dup = (70, 1500, 4098)                                                   # three workgroups
    for n in dup:
        W[n] = W[70]
    st = State(B, V, 4, 0)
    st.seen[1, 70] = 1                                                       # sample 1 has seen the lowest: its logit is positive, so it falls
    want, bound, _ = HR.head_expect(X, W, st.seen, 1.3)
    assert_determined(want[:1], bound[:1], "ties", equals=dup)
    assert float(want[1, 70]) > 0 and float(want[1, 70]) < float(want[1, 1500]) == float(want[1, 4098])
    assert_determined(want[1:], bound[1:], "ties, lowest seen", equals=dup[1:])
    assert HR.argmax_lowest(want).tolist() == [70, 1500]
    assert run(ho, X, W, st, penalty=1.3).tolist() == [70, 1500]


def test_select_with_every_logit_negative_and_the_top_one_seen(ho):
    B, V, K = 1, 1000, 256
    X, W = head_inputs(B, V, K, seed=31)
    x = X[0].float()
    W = (W.float() - 12.0 * x[None] / float(x.pow(2).sum())).bfloat16()      # every logit moves by -12
    l = X.double() @ W.double().T
    assert bool((l < 0).all())
    top2 = l.topk(2, -1).indices[0].tolist()
    st = State(B, V, 4, 0)
    st.seen[0, top2[0]] = 1
    pen = 1.0 + 2.0 * float(l[0, top2[0]] - l[0, top2[1]]) / float(l[0, top2[0]].abs())      # `* penalty` takes the top one below the second
    want, bound, _ = HR.head_expect(X, W, st.seen, pen)
    assert_determined(want, bound, "all negative")
    assert int(HR.argmax_lowest(want)) != top2[0]
    assert run(ho, X, W, st, penalty=pen).tolist() == HR.argmax_lowest(want).tolist()


# ---------------------------------------------------------------------------------------------------------------- bookkeeping
def test_bookkeeping_of_one_token_and_nothing_else_written(ho):
    B, V, K = 3, 1000, 256
    X, W = head_inputs(B, V, K, seed=41)
    winners = [5, 600, 999]
    for b, n in enumerate(winners):
        plant(W, X, b, n, 9.0)
    want, bound, _ = HR.head_expect(X, W)
    assert_determined(want, bound, "bookkeeping")
    st = State(B, V, 6, 2, eos=(600, 77), done=[0, 0, 1])                   # two end ids, one of them sample 1's token; sample 2 is done
    st.seen_buf.fill_(SEEN_SENTINEL)                                         # (non-zero: seen; the penalty is 1)
    before = st.snapshot()
    run(ho, X, W, st, pad=3)
    ref = {k: (None if v is None else v.cpu()) for k, v in before.items()}
    col = HR.select_reference(torch.tensor(winners), 2, ref["token"], ref["seq"][:, :6], ref["lengths"], ref["done"], [600, 77], 3, ref["seen"][:, :V])
    assert st.token.tolist() == [5, 600, 3] == ref["token"].tolist()
    assert torch.equal(st.seq_buf.cpu(), ref["seq"]) and int((st.seq_buf != -7).sum()) == 3        # the counter's column and nowhere else
    assert st.lengths.tolist() == [1, 1, 0] and st.done.tolist() == [0, 1, 1] and st.step.tolist() == [col] == [3]
    changed = st.seen_buf != SEEN_SENTINEL
    assert changed.sum(-1).tolist() == [1, 1, 1] and torch.equal(st.seen_buf.cpu(), ref["seen"])    # exactly one byte per row
    assert [int(st.seen_buf[b, t]) for b, t in enumerate([5, 600, 3])] == [1, 1, 1]
    # a counter outside the columns: no column is written, the rest goes on, the counter still advances
    for col in (6, -4, 2 ** 31 - 2):
        st2 = State(B, V, 6, col)
        run(ho, X, W, st2, pad=3)
        torch.cuda.synchronize()
        assert int((st2.seq_buf != -7).sum()) == 0 and st2.token.tolist() == winners and st2.step.tolist() == [col + 1]
        assert st2.lengths.tolist() == [1, 1, 1]


def test_three_captured_calls_replay_as_three_eager_calls(ho):
    B, V, K = 2, 1000, 256
    X, W = head_inputs(B, V, K, seed=51)
    ws = torch.empty((ho.workspace_floats(B, V),), device=DEV, dtype=torch.float32)

    def three(st):
        for _ in range(3):                                                   # the penalty makes each call's winner fall: three tokens
            run_nocopy(st)

    def run_nocopy(st):
        ho.logits_argmax(X, W, ws, seen=st.seen, penalty=50.0, step=st.step)
        ho.select(ws, st.step, st.token, st.seq, st.lengths, st.done, 0, V, eos=st.eos, seen=st.seen)

    eager = State(B, V, 5, 1, eos=(V - 1,))
    three(eager)
    torch.cuda.synchronize()
    st = State(B, V, 5, 1, eos=(V - 1,))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run_nocopy(State(B, V, 5, 1, eos=(V - 1,)))                          # the warm-up a capture needs, on a state of its own
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        three(st)
    assert int((st.seq_buf != -7).sum()) == 0                                # a capture runs nothing
    g.replay()
    torch.cuda.synchronize()
    a, b = eager.snapshot(), st.snapshot()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert st.step.tolist() == [4] and len(set(st.seq[0, 1:4].tolist())) == 3 and st.lengths.tolist() == [3, 3]


# ---------------------------------------------------------------------------------------------------------------- hand-off
SEED = 5


def tiny_model():
    from transformers import Qwen2ForCausalLM
    cfg = QR.library_config(256, 2, 1, 512, 3)
    cfg._attn_implementation = "sdpa"
    torch.manual_seed(0)
    model = Qwen2ForCausalLM(cfg).eval().requires_grad_(False)
    model.model.load_state_dict(QR.random_stack_state_dict(model.model, seed=SEED), strict=True)
    return model.to(device=DEV, dtype=torch.bfloat16)


def test_hip_generate_with_the_hip_head():
    """The tiny Qwen2ForCausalLM of tests/test_qwen_decode_gpu.py (hidden 256, 3 layers, 64 tokens), B = 2 with sample 0 right-padded, 9 new
    tokens, penalty 1.05 with a temperature and a top-k warper in the list"""
    from transformers.generation.logits_process import (MinLengthLogitsProcessor, RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper,
                                                        TopKLogitsWarper)
    from x2i_amd.handoff import HipGenerate, find_decoder
    model = tiny_model()
    B, S, T = 2, 77, 9
    ids = torch.randint(0, 64, (B, S), generator=torch.Generator().manual_seed(6)).to(DEV)
    mask = torch.ones((B, S), dtype=torch.long, device=DEV)
    mask[0, 50:] = 0
    hg = HipGenerate(model)
    procs = [RepetitionPenaltyLogitsProcessor(1.05)]
    before = hg.generate(model, max_new_tokens=T, eos_token_id=None, logits_processor=procs, graph=True, input_ids=ids, attention_mask=mask)
    fused = [TemperatureLogitsWarper(0.7), RepetitionPenaltyLogitsProcessor(1.05), TopKLogitsWarper(5)]
    W = model.lm_head.weight
    runs = {}
    for graph in (False, True):
        out = runs[graph] = hg.generate(model, max_new_tokens=T, eos_token_id=None, logits_processor=fused, graph=graph, hip_head=True, input_ids=ids,
                                        attention_mask=mask)
        assert "forward" not in find_decoder(model).__dict__                                 # the decoder's forward is restored
        assert torch.equal(out.prompt, before.prompt)
        assert out.answer.shape == (B, 4, T - 1, 256) and out.answer.dtype == torch.bfloat16
        assert out.sequences.shape == (B, S + T) and torch.equal(out.sequences[:, :S], ids) and out.lengths.tolist() == [T, T]
        first = out.prompt[:, -1][torch.arange(B), torch.tensor([49, S - 1])]
        for t in range(T):
            x = first if t == 0 else out.answer[:, -1, t - 1]
            want, bound, _ = HR.head_expect(x, W, HR.seen_of(out.sequences[:, :S + t], 64), 1.05)
            gap, allow = HR.margin(want, bound)
            assert bool((gap > allow).all()), "seed %d, token %d: the float64 margin %s does not exceed twice the bound %s -- an unlucky seed, " \
                "not a wrong token: choose another" % (SEED, t, gap.tolist(), allow.tolist())
            assert torch.equal(HR.argmax_lowest(want), out.sequences[:, S + t]), t
        assert torch.equal(out.answer[:, 0], model.model.embed_tokens.weight[out.sequences[:, S:S + T - 1]])
    assert torch.equal(runs[True].sequences, runs[False].sequences) and torch.equal(runs[True].answer, runs[False].answer)
    # an end token: sample 1's third token ends it; pad follows, the lengths say so, and the host's look every 2 steps stops the loop early
    seq = runs[False].sequences
    eos = int(seq[1, S + 2])
    stop0 = [t for t in range(T) if int(seq[0, S + t]) == eos]
    n1 = min(t for t in range(T) if int(seq[1, S + t]) == eos) + 1
    n0 = stop0[0] + 1 if stop0 else T
    n = max(n0, n1)
    for graph in (False, True):
        out = hg.generate(model, max_new_tokens=T, eos_token_id=[eos, 62], pad_token_id=63, logits_processor=fused, graph=graph, check_every=2,
                          hip_head=True, input_ids=ids, attention_mask=mask)
        n0g = min([n0] + [t + 1 for t in range(T) if int(seq[0, S + t]) == 62])
        n1g = min([n1] + [t + 1 for t in range(T) if int(seq[1, S + t]) == 62])
        assert out.lengths.tolist() == [n0g, n1g] and out.sequences.shape == (B, S + max(n0g, n1g)) and out.answer.shape[2] == max(n0g, n1g) - 1
        assert torch.equal(out.sequences[1, S:S + n1g], seq[1, S:S + n1g]) and bool((out.sequences[1, S + n1g:] == 63).all())
        assert torch.equal(out.sequences[0, S:S + n0g], seq[0, S:S + n0g]) and bool((out.sequences[0, S + n0g:] == 63).all())
    # an unsupported processor is refused by name before anything runs, and forward stays the model's own
    with pytest.raises(ValueError, match="MinLengthLogitsProcessor"):
        hg.generate(model, max_new_tokens=T, logits_processor=fused + [MinLengthLogitsProcessor(3, 1)], hip_head=True, input_ids=ids, attention_mask=mask)
    assert "forward" not in find_decoder(model).__dict__
    # the default, in the same process, returns what it returned before
    after = hg.generate(model, max_new_tokens=T, eos_token_id=None, logits_processor=procs, graph=True, input_ids=ids, attention_mask=mask)
    assert torch.equal(after.sequences, before.sequences) and torch.equal(after.answer, before.answer) and torch.equal(after.prompt, before.prompt)
    # the constructor's flag is the default of the call
    assert torch.equal(HipGenerate(model, hip_head=True).generate(model, max_new_tokens=T, logits_processor=fused, input_ids=ids,
                                                                 attention_mask=mask).sequences, runs[True].sequences)


class StubProcessor:
    """a tokenizer of 60 words for the multi-turn conditioner: ids 2 .. 61 are the 'words' w2 .. w61, a turn of the history is its words"""

    def apply_chat_template(self, history, tokenize=False, add_generation_prompt=True):
        return " | ".join(c["text"] for m in history for c in m["content"] if c["type"] == "text")

    def __call__(self, text, images=None, return_tensors="pt"):
        from transformers import BatchFeature
        ids = [[int(w[1:]) for w in t.replace("|", " ").split()] for t in text]
        return BatchFeature({"input_ids": torch.tensor(ids), "attention_mask": torch.ones((len(ids), len(ids[0])), dtype=torch.long)})

    def batch_decode(self, ids, skip_special_tokens=True):
        return [" ".join("w%d" % min(max(int(i), 2), 61) for i in row) for row in ids]


def test_multi_turn_conditioner_on_hip_generate():
    from transformers import GenerationConfig
    from x2i_amd.handoff import HipGenerate
    from x2i_amd.infer.inference_multi_turn import MultiTurnConditioner
    model = tiny_model()
    model.generation_config = GenerationConfig(do_sample=True, top_k=1, temperature=0.5, repetition_penalty=1.05, eos_token_id=1, pad_token_id=0)
    cond = MultiTurnConditioner(None, DEV, hip_generate=True, hip_head=True, model=model, processor=StubProcessor())
    prompts = ["w5 w9 w33 w12 w7 w40 w21", "w3 w3 w8"]
    direct = HipGenerate(model, hip_head=True)
    text = []
    for turn, p in enumerate(prompts):
        slab, answer = cond(text_prompt=p)
        text.append(p)
        ids = StubProcessor()([" | ".join(text)])["input_ids"].to(DEV)
        S = ids.shape[1]
        gc = model.generation_config
        want = direct.generate(model, max_new_tokens=64, eos_token_id=gc.eos_token_id, pad_token_id=gc.pad_token_id,
                               logits_processor=model._get_logits_processor(gc, input_ids_seq_length=S, device=DEV), input_ids=ids,
                               attention_mask=torch.ones_like(ids))
        assert want.answer.shape[2] > 0 and torch.equal(slab, torch.cat([want.prompt, want.answer], dim=2))
        assert answer == StubProcessor().batch_decode(want.sequences[:, S:])[0]
        text.append(answer)
        assert cond.history[-1] == {"role": "assistant", "content": [{"type": "text", "text": answer}]} and len(cond.history) == 2 * (turn + 1)
    # the second turn's prompt held the first turn's answer: its ids are prompt 0, answer 0, prompt 1
    assert ids.shape[1] == 7 + len(text[1].split()) + 3 and text[1] in " | ".join(text[:3])
    with pytest.raises(ValueError, match="hip_generate"):
        MultiTurnConditioner(None, DEV, hip_head=True, model=model, processor=StubProcessor())
