"""HipGenerate(hip_head=True, sample=True) on a tiny random Qwen2ForCausalLM (hidden 256, 3 layers, 300 tokens; built as
tests/test_qwen_head_gpu.py builds its own): a sampling generation_config on the HIP path -- reproducible under a seed, the same eager and
replayed, greedy under top_k = 1, and the last token checked against the float64 reference of tests/sample_ref.py."""
import numpy as np
import pytest
import torch

from tests import qwen_ref as QR
from tests import sample_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 5
V, B, S, T = 300, 2, 21, 12
NO_CHECKPOINT = "/nonexistent/checkpoint/that/must/never/be/read"
SEEDS = (1, 2)      # two seeds whose sequences differ (pinned)


@pytest.fixture(scope="module")
def model():
    from transformers import GenerationConfig, Qwen2ForCausalLM
    cfg = QR.library_config(256, 2, 1, 512, 3, vocab=V)
    cfg._attn_implementation = "sdpa"
    torch.manual_seed(0)
    m = Qwen2ForCausalLM(cfg).eval().requires_grad_(False)
    m.model.load_state_dict(QR.random_stack_state_dict(m.model, seed=SEED), strict=True)
    m = m.to(device=DEV, dtype=torch.bfloat16)
    m.generation_config = GenerationConfig(do_sample=True, temperature=0.7, top_k=20, top_p=0.9, repetition_penalty=1.05, eos_token_id=None,
                                           pad_token_id=0)
    return m


@pytest.fixture(scope="module")
def prompt():
    ids = torch.randint(0, V, (B, S), generator=torch.Generator().manual_seed(6)).to(DEV)
    mask = torch.ones((B, S), dtype=torch.long, device=DEV)
    mask[0, 15:] = 0
    return dict(input_ids=ids, attention_mask=mask)


def run(hg, model, prompt, gc=None, **kw):
    gc = model.generation_config if gc is None else gc
    procs = model._get_logits_processor(gc, input_ids_seq_length=S, device=DEV)
    return hg.generate(model, max_new_tokens=T, eos_token_id=None, pad_token_id=0, logits_processor=procs, generation_config=gc, **kw, **prompt)


def test_a_seed_gives_its_sequences_again_eager_or_replayed_and_another_seed_gives_others(model, prompt):
    from x2i_amd.handoff import HipGenerate
    hg = HipGenerate(model, hip_head=True, sample=True)
    a = run(hg, model, prompt, seed=SEEDS[0])
    assert a.sequences.shape == (B, S + T) and a.lengths.tolist() == [T, T] and bool(((0 <= a.sequences) & (a.sequences < V)).all())
    assert hg._rng == [SEEDS[0], T]                                  # the stream went on by the tokens generated
    b = run(hg, model, prompt, seed=SEEDS[0])
    assert torch.equal(a.sequences, b.sequences) and torch.equal(a.answer, b.answer)
    e = run(hg, model, prompt, seed=SEEDS[0], graph=False)
    assert torch.equal(a.sequences, e.sequences) and torch.equal(a.answer, e.answer)
    c = run(hg, model, prompt, seed=SEEDS[1])
    assert not torch.equal(a.sequences, c.sequences)
    d = run(hg, model, prompt)                                       # no seed: the stream goes on, at offset T
    assert hg._rng == [SEEDS[1], 2 * T] and not torch.equal(d.sequences, c.sequences)
    # the constructor's seed is the first call's
    assert torch.equal(run(HipGenerate(model, hip_head=True, sample=True, seed=SEEDS[0]), model, prompt).sequences, a.sequences)


def test_top_k_1_is_the_greedy_hip_head_run_token_for_token(model, prompt):
    from transformers import GenerationConfig
    from x2i_amd.handoff import HipGenerate
    gc = GenerationConfig(do_sample=True, temperature=0.7, top_k=1, top_p=0.9, repetition_penalty=1.05, eos_token_id=None, pad_token_id=0)
    hg = HipGenerate(model, hip_head=True)
    greedy = run(hg, model, prompt, gc=gc)
    sampled = run(hg, model, prompt, gc=gc, sample=True, seed=3)
    assert torch.equal(greedy.sequences, sampled.sequences) and torch.equal(greedy.answer, sampled.answer)
    # under another top_k the captured greedy step is not replayed: the key of the graphs holds the three values
    other = run(hg, model, prompt, sample=True, seed=3)
    assert not torch.equal(other.sequences, sampled.sequences)
    assert torch.equal(run(hg, model, prompt, gc=gc).sequences, greedy.sequences)


def test_the_last_token_passes_the_verdict_against_the_score_buffer(model, prompt):
    from x2i_amd import sample_binding as sb
    from x2i_amd.handoff import HipGenerate
    gc = model.generation_config
    hg = HipGenerate(model, hip_head=True, sample=True)
    out = run(hg, model, prompt, seed=11)
    run(hg, model, prompt)                                           # a second call, at offset T: what the state holds is this one
    out = run(hg, model, prompt)
    st = hg._state
    seed, offset = (int(x) for x in st["h_rng"].tolist())
    col = int(st["h_step"].item()) - 1
    assert (seed, offset, col) == (11, 2 * T, S + T - 1)
    logits = st["h_logits"].cpu().numpy()
    diag = torch.zeros((B, 4), device=DEV)
    scratch = dict(step=torch.zeros(1, device=DEV, dtype=torch.int32), token=torch.zeros(B, device=DEV, dtype=torch.long),
                   sequences=torch.zeros((B, 1), device=DEV, dtype=torch.long), lengths=torch.zeros(B, device=DEV, dtype=torch.long),
                   done=torch.zeros(B, device=DEV, dtype=torch.uint8))
    sb.select(st["h_logits"], st["h_ws"], pad=0, temperature=gc.temperature, top_k=gc.top_k, top_p=gc.top_p, rng=st["h_rng"], diag=diag, **scratch)
    diag = diag.cpu().numpy()
    assert torch.equal(scratch["token"], out.sequences[:, -1])      # the launch again, outside the loop: the token the loop wrote
    for b in range(B):
        ref = R.select(logits[b], gc.temperature, gc.top_k, gc.top_p)
        u = R.uniform(seed, offset, col, b)
        assert diag[b, 3].view(np.uint32) == u.view(np.uint32)
        assert ref.margin > 0 and R.admitted(ref, u).size == 1, "an unlucky seed, not a wrong token: choose another"
        bad = R.verdict(ref, int(out.sequences[b, -1]), u, diag[b, 0], diag[b, 2])
        assert not bad, bad
        assert 1 < ref.count <= 20


def test_without_sample_the_config_is_refused_and_hip_sample_needs_hip_head(model, prompt):
    from x2i_amd.handoff import HipGenerate
    from x2i_amd.infer.inference_multi_turn import MultiTurnConditioner
    from x2i_amd.infer.inference_qwenvl import QwenVLConditioner
    hg = HipGenerate(model, hip_head=True)
    with pytest.raises(ValueError, match="greedy decoding only"):
        run(hg, model, prompt)
    with pytest.raises(ValueError, match="greedy decoding only"):
        run(hg, model, prompt, sample=False)
    with pytest.raises(ValueError, match="not without hip_head"):
        run(HipGenerate(model), model, prompt, sample=True)
    for make in (lambda: QwenVLConditioner(NO_CHECKPOINT, "cpu", hip_generate=True, hip_sample=True),
                 lambda: MultiTurnConditioner(NO_CHECKPOINT, "cpu", hip_generate=True, hip_sample=True),
                 lambda: MultiTurnConditioner(NO_CHECKPOINT, "cpu", hip_head=True, hip_sample=True, model=model, processor=object())):
        with pytest.raises(ValueError, match="--hip_sample"):
            make()
    from transformers.generation.logits_process import MinPLogitsWarper
    with pytest.raises(ValueError, match="MinPLogitsWarper"):
        hg.generate(model, max_new_tokens=T, logits_processor=[MinPLogitsWarper(0.1)], sample=True, **prompt)
