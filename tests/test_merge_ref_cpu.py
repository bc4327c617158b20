"""CPU-side checks of the prompt merge (no GPU): the torch restatement tests/merge_ref.py against the literal torch forms of the two chat
models (tests/test_merge_gpu.py's tiny models: scatter over stacked aranges, slice assignment per bound, masked assignment over the
flattened batch), the plan constructors' host side, the extension header include/x2i_merge.h (its prototypes against the binding: tests/test_extension_boundary_cpu.py), every refusal of its two entry points, the wiring of --hip_decoder into the MiniCPM-o and InternVL conditioners, and the
InternVL query builder against the strings recorded from the reference (tests/golden/internvl_query.json)."""
import ctypes as C
import json
import os
from types import SimpleNamespace

import pytest
import torch

from tests import merge_ref as MR
from tests.test_merge_gpu import HID, TinyInternVL, TinyMiniCPM, internvl_inputs, minicpm_inputs, to_device  # (helpers; its tests are marked gpu)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(t):
    return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("chunk_input", [True, False])
def test_reference_is_the_minicpm_scatter_and_slice_assignments(chunk_input):
    """two samples: one without features, one with three image bounds and two audio bounds; token rows times scale_emb = 12"""
    from x2i_amd.merge import MergePlan, host_ints
    model = TinyMiniCPM(chunk_input=chunk_input).bfloat16()
    inputs = to_device(minicpm_inputs(chunk_input), "cpu", torch.bfloat16)
    own = model.merged(inputs)
    B, S = inputs["input_ids"].shape
    image_bound, audio_bounds = host_ints(inputs["image_bound"], inputs["audio_bounds"])
    src, counts = MergePlan.src_from_bounds(B, S, image_bound, audio_bounds, vision_rows=[0, 12], audio_rows=[0, 5])
    src = torch.from_numpy(src)
    assert counts == [12, 5] and torch.equal(src, MR.src_from_bounds_ref(B, S, image_bound, audio_bounds))
    assert int((src >= 0).sum()) == 17 and int((src[:S] >= 0).sum()) == 0          # sample 0 takes no feature row
    vision = torch.cat([r for r in model.vision_rows(inputs) if len(r)]).reshape(-1, HID)
    audio = torch.cat([e for sample in model.get_audio_embedding(inputs) for e in sample])
    table = model.llm.model.embed_tokens.weight
    out, flag = MR.merge_ref(inputs["input_ids"], src, table, 12.0, vision, audio)
    assert flag == 0 and torch.equal(bits(out), bits(own))
    assert not torch.equal(bits(out), bits(MR.merge_ref(inputs["input_ids"], src, table, 1.0, vision, audio)[0]))
    # overwrite mode on the scaled token rows is the same merge
    over, _ = MR.merge_ref(inputs["input_ids"], src, None, 1.0, vision, audio, out=table[inputs["input_ids"]] * 12.0)
    assert torch.equal(bits(over), bits(own))


def test_reference_is_the_internvl_masked_assignment():
    model = TinyInternVL().bfloat16()
    inputs = to_device(internvl_inputs(), "cpu", torch.bfloat16)
    own = model.merged(inputs["pixel_values"], inputs["input_ids"])
    src, total = MR.rank_ref(inputs["input_ids"], model.CTX)
    hit = inputs["input_ids"].reshape(-1) == model.CTX
    assert total == 12 and src[hit].tolist() == list(range(12)) and bool((src[~hit] == -1).all())
    out, flag = MR.merge_ref(inputs["input_ids"], src, model.language_model.get_input_embeddings().weight, 1.0,
                             model.extract_feature(inputs["pixel_values"]).reshape(-1, HID))
    assert flag == 0 and torch.equal(bits(out), bits(own))


def test_reference_zeroes_out_of_range_rows_and_flags_them():
    g = torch.Generator().manual_seed(1)
    table, feat = torch.randn((10, 8), generator=g).bfloat16(), torch.randn((3, 8), generator=g).bfloat16()
    ids = torch.tensor([[1, 10, 2, 3, 4]])
    src = torch.tensor([-1, -1, 0, 3, 2 | (1 << 30)], dtype=torch.int32)
    out, flag = MR.merge_ref(ids, src, table, 1.0, feat, None)
    assert flag == 1 and torch.equal(out[0, 0], table[1]) and torch.equal(out[0, 2], feat[0])
    assert bool((out[0, 1] == 0).all()) and bool((out[0, 3] == 0).all()) and bool((out[0, 4] == 0).all())


# ---------------------------------------------------------------------------------------------------------------- the plan's host side
def test_host_ints_keeps_the_nesting_and_cpu_tensors_need_no_copy(monkeypatch):
    from x2i_amd import merge
    calls = []
    real = torch.cat
    monkeypatch.setattr(merge.torch, "cat", lambda *a, **k: calls.append(1) or real(*a, **k))
    got = merge.host_ints([torch.tensor([[1, 3], [5, 6]]), []], None, [[2, 2]], [torch.zeros((0, 2), dtype=torch.long)])
    assert got == [[[[1, 3], [5, 6]], []], None, [[2, 2]], [[]]] and calls == []


def test_src_from_bounds_refuses_by_name():
    from x2i_amd.merge import MergePlan
    f = MergePlan.src_from_bounds
    with pytest.raises(ValueError, match=r"bound \[4, 9\) of sample 1 does not lie in a prompt of 8 rows"):
        f(2, 8, [[], [[4, 9]]])
    with pytest.raises(ValueError, match=r"bound \[5, 4\)"):
        f(1, 8, [[[5, 4]]])
    with pytest.raises(ValueError, match="3 bound lists for a batch of 2"):
        f(2, 8, [[], [], []])
    with pytest.raises(ValueError, match=r"ask for \[0, 2\] audio rows per sample and the features have \[0, 3\]"):
        f(2, 8, None, [[], [[1, 3]]], audio_rows=[0, 3])
    # a later bound wins where two overlap, audio over vision
    src, counts = f(1, 8, [[[0, 4]]], [[[2, 3]]])
    assert src.tolist() == [0, 1, 1 << 30, 3, -1, -1, -1, -1] and counts == [4, 1]


# ---------------------------------------------------------------------------------------------------------------- boundary
def test_the_headers_constants_are_the_bindings_and_the_references():
    from x2i_amd import merge_ops
    text = open(os.path.join(ROOT, "include", "x2i_merge.h")).read()
    assert "#define X2I_MERGE_RANK_CHUNK %d\n" % merge_ops.RANK_CHUNK in text
    assert "#define X2I_MERGE_SRC_ARRAY_BIT %d\n" % merge_ops.SRC_ARRAY_BIT in text and "#define X2I_MERGE_SRC_ROW_MASK 0x%x\n" % merge_ops.SRC_ROW_MASK in text
    assert MR.ARRAY_BIT == merge_ops.SRC_ARRAY_BIT and MR.ROW_MASK == merge_ops.SRC_ROW_MASK
    assert [merge_ops.rank_workspace_ints(n) for n in (1, 2048, 2049, 8 * 32768)] == [1, 1, 2, 128]


def test_entry_points_validate_their_arguments_without_a_gpu():
    from x2i_amd import merge_ops
    lib = merge_ops.load()
    fake = C.c_void_p(0x1000)  # never dereferenced: validation fails first
    odd8, odd4, odd2 = C.c_void_p(0x1008), C.c_void_p(0x1004), C.c_void_p(0x1002)
    err = lambda: lib.x2i_last_error()
    rk = lambda **kw: lib.x2i_merge_rank_i32(*[kw.get(k, d) for k, d in (
        ("ids", fake), ("n", 5000), ("ph", 7), ("src", fake), ("total", fake), ("ws", fake), ("wsn", 3), ("st", None))])
    assert rk(n=0) < 0 and b"n=0" in err()
    assert rk(n=(1 << 24) + 1, wsn=1 << 20) < 0 and b"2^24" in err()
    assert rk(wsn=2) < 0 and b"workspace too small" in err()
    assert rk(ids=odd4) < 0 and b"aligned" in err()
    for k in ("src", "total", "ws"):
        assert rk(**{k: odd2}) < 0 and b"aligned" in err()
    for k in ("ids", "src", "total", "ws"):
        assert rk(**{k: None}) < 0 and b"null" in err()
    em = lambda **kw: lib.x2i_embed_merge_bf16(*[kw.get(k, d) for k, d in (
        ("ids", fake), ("src", fake), ("table", fake), ("ldt", 64), ("V", 100), ("scale", 1.0), ("f0", fake), ("ldf0", 64), ("n0", 5), ("f1", fake),
        ("ldf1", 72), ("n1", 6), ("out", fake), ("ldo", 64), ("obs", 64 * 77 * 3), ("err", fake), ("B", 2), ("S", 77), ("H", 64), ("st", None))])
    assert em(B=0) < 0 and b"B=0" in err()
    assert em(S=0) < 0 and em(B=1 << 16, S=1 << 15, obs=1 << 40) < 0 and b"2^30" in err()
    assert em(H=60) < 0 and b"H=60" in err()
    assert em(H=0) < 0 and em(V=0) < 0 and b"V=0" in err()
    assert em(n0=-1) < 0 and em(f1=None) < 0 and b"0 without an array" in err()
    for bad in (float("inf"), float("nan")):
        assert em(scale=bad) < 0 and b"scale" in err()
    for k in ("ldt", "ldf0", "ldf1", "ldo"):
        assert em(**{k: 56}) < 0 and b"row stride" in err()
        assert em(**{k: 68}) < 0 and b"row stride" in err()
    assert em(obs=76 * 64 + 56) < 0 and em(obs=64 * 76) < 0 and b"holds S rows" in err()
    for k in ("table", "f0", "f1", "out"):
        assert em(**{k: odd8}) < 0 and b"aligned" in err()
    assert em(ids=odd4) < 0 and em(src=odd2) < 0 and em(err=odd2) < 0 and b"aligned" in err()
    assert em(out=None) < 0 and em(err=None) < 0 and b"null" in err()
    assert em(ids=None) < 0 and b"ids with a table" in err()
    assert em(table=None, src=None) < 0 and b"overwrite mode" in err()


# ---------------------------------------------------------------------------------------------------------------- the query strings
def test_query_builder_gives_the_references_strings():
    from x2i_amd.infer.inference_internvl import IMG_CONTEXT_TOKEN, build_query
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "internvl_query.json"), encoding="utf-8"))["cases"]
    assert [c["num_patches_list"] for c in cases] == [[], [1], [13]]
    for c in cases:
        assert build_query(c["text_prompt"], c["num_patches_list"]) == c["query"], c["name"]
        assert c["query"].count(IMG_CONTEXT_TOKEN) == 256 * sum(c["num_patches_list"])
    assert "<image>" not in cases[2]["query"] and cases[0]["query"].endswith("<|im_start|>assistant\n")


# ---------------------------------------------------------------------------------------------------------------- wiring
def test_generate_positions_are_the_installed_librarys():
    """left, right and no padding; the padding's position is the library's own (it differs between its major versions)"""
    from tests.test_merge_gpu import tiny_causal_lm
    from x2i_amd.handoff import generate_positions
    mask = torch.tensor([[1, 1, 1, 0, 0, 0], [0, 0, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1]])
    want = tiny_causal_lm(1)._prepare_position_ids_for_generation(torch.zeros((3, 6), dtype=torch.long), {"attention_mask": mask})
    assert torch.equal(generate_positions(mask), want) and generate_positions(None) is None
    assert generate_positions(mask, pad_position=1)[0].tolist() == [0, 1, 2, 1, 1, 1]


def test_harness_takes_hip_decoder_for_both_models_and_the_scripts_hand_it_on(monkeypatch):
    from x2i_amd.infer import harness, inference_internvl, inference_minicpm
    for family, mod, cls in (("minicpm", inference_minicpm, "MiniCPMConditioner"), ("internvl", inference_internvl, "InternVLConditioner")):
        p = harness.build_parser(family)
        assert p.parse_args([]).hip_decoder is False and p.parse_args(["--hip_decoder"]).hip_decoder is True
        help_text = " ".join(p.format_help().split())
        assert "HipMiniCPMPrompt" in help_text and "HipInternVLPrompt" in help_text and "no lm_head runs" in help_text
        seen = {}
        monkeypatch.setattr(mod, cls, lambda *a, **kw: seen.update(kw) or "cond")
        monkeypatch.setattr(mod, "Harness", lambda *a, **kw: SimpleNamespace(run_tasks=lambda tasks: None))
        monkeypatch.setattr(mod.torch.cuda, "set_device", lambda d: None)
        mod.main(["--hip_decoder", "--hip_vision"])
        assert seen["hip_decoder"] is True and seen["hip_vision"] is True and seen["prefill_only"] is True and not seen["use_answer"]
        mod.main(["--full_generate"])
        assert seen["hip_decoder"] is False and seen["prefill_only"] is False


def test_conditioners_take_hip_decoder_and_refuse_it_with_full_generate_or_use_answer():
    from x2i_amd.handoff import HipInternVLPrompt, HipMiniCPMPrompt
    from x2i_amd.infer.inference_internvl import InternVLConditioner, build_query
    from x2i_amd.infer.inference_minicpm import MiniCPMConditioner
    boom = SimpleNamespace()          # a model that must not be touched: the refusal comes first
    for kw in (dict(prefill_only=False), dict(use_answer=True)):
        with pytest.raises(ValueError, match="--hip_decoder serves the prompt pass only"):
            MiniCPMConditioner(None, "cpu", model=boom, hip_decoder=True, **kw)
        with pytest.raises(ValueError, match="--hip_decoder serves the prompt pass only"):
            InternVLConditioner(None, "cpu", model=boom, hip_decoder=True, **kw)
    cond = MiniCPMConditioner(None, "cpu", model=TinyMiniCPM(), hip_decoder=True)
    assert isinstance(cond.prompt, HipMiniCPMPrompt) and cond.slab is None and cond.vision is cond.resampler is cond.audio is None
    assert MiniCPMConditioner(None, "cpu", model=TinyMiniCPM()).prompt is None

    class Tok:
        def convert_tokens_to_ids(self, t):
            return 60

        def __call__(self, q, **kw):
            self.q, self.kw = q, kw
            out = SimpleNamespace(input_ids="ids", attention_mask="mask")
            out.to = lambda d: out
            return out
    for hip in (True, False):
        model, tok = TinyInternVL(), Tok()
        cond = InternVLConditioner(None, "cpu", model=model, tokenizer=tok, hip_decoder=hip)
        assert isinstance(cond.prompt, HipInternVLPrompt) == hip and (cond.slab is None) == hip
        cond.hidden_states = lambda pv, ids, mask: (pv, ids, mask)
        assert cond(text_prompt="a cat") == (None, "ids", "mask")
        # every mode tokenises the reference's query, and the model knows its context token
        assert tok.q == build_query("a cat", [], 4) and tok.kw["max_length"] == 512 and model.img_context_token_id == 60


def test_prompt_handoffs_install_remove_and_refuse_by_name():
    from x2i_amd._lib import X2IError
    from x2i_amd.handoff import HipInternVLPrompt, HipMiniCPMPrompt
    for make, model, inputs in ((HipInternVLPrompt, TinyInternVL(), internvl_inputs()), (HipMiniCPMPrompt, TinyMiniCPM(), minicpm_inputs(True))):
        own = model.generate
        model.marker = 1
        before = dict(model.__dict__)
        h = make(model)
        assert model.__dict__ == before and h.C == 3 and h.stack.embed_tokens.weight.dtype == torch.bfloat16
        h.install().install()
        assert model.__dict__["generate"] == h._generate
        h.remove()
        h.remove()
        assert model.__dict__ == before and model.generate == own
        # restored after an exception too: on the CPU the first launch refuses (there is no CPU fallback)
        with pytest.raises(X2IError, match="must live on the GPU"):
            with h:
                model.generate(**inputs)
        assert model.__dict__ == before and h.calls == 0
        # an instance that already carries a generate of its own gets exactly that one back
        mine = lambda **kw: "mine"
        model.generate = mine
        with h:
            assert model.generate is not mine
        assert model.__dict__["generate"] is mine
        del model.generate
        with pytest.raises(ValueError, match="needs input_ids"):
            h._generate()
        model.train()
        with pytest.raises(ValueError, match="training mode"):
            make(model)
        model.eval()
    with pytest.raises(RuntimeError, match="no language model"):
        HipInternVLPrompt(SimpleNamespace(extract_feature=lambda x: x))
    with pytest.raises(RuntimeError, match="no extract_feature"):
        HipInternVLPrompt(SimpleNamespace())
    with pytest.raises(RuntimeError, match="no model.vpm"):
        HipMiniCPMPrompt(SimpleNamespace())
    h = HipMiniCPMPrompt(TinyMiniCPM())
    with pytest.raises(ValueError, match="stream=True and precomputed vision_hidden_states"):
        h._generate(input_ids=torch.zeros((1, 4), dtype=torch.long), stream=True)
    model = TinyInternVL()
    model.img_context_token_id = None
    with pytest.raises(ValueError, match="img_context_token_id is not set"):
        HipInternVLPrompt(model).prompt(torch.zeros((1, 4), dtype=torch.long), pixel_values=torch.zeros((1, 3, 4, 4)))
