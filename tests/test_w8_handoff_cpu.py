"""CPU checks of the --hip_w8 option: the harness declares it, both inference scripts refuse it without --hip_generate before any checkpoint
is read, and Qwen2DecoderStack.decode_step(w8=True) refuses to run without a pack."""
import pytest
import torch

NO_CHECKPOINT = "/nonexistent/checkpoint/that/must/never/be/read"


def test_harness_takes_the_hip_w8_flag_and_the_defaults_stay():
    from x2i_amd.infer.harness import build_parser
    p = build_parser("qwenvl")
    a = p.parse_args(["--synthetic"])
    assert a.hip_w8 is False and a.hip_head is False and a.hip_generate is False
    a = p.parse_args(["--synthetic", "--hip_generate", "--hip_w8"])
    assert a.hip_w8 is True and a.hip_generate is True and a.hip_head is False
    assert p.parse_args(["--synthetic", "--hip_generate", "--hip_head", "--hip_w8"]).hip_w8 is True
    help_text = " ".join(p.format_help().split())
    assert "--hip_w8" in help_text and "e4m3" in help_text and "6.5 GB" in help_text
    # declared next to --hip_head
    names = [a.dest for a in p._actions]
    assert names.index("hip_w8") == names.index("hip_head") + 1


def test_hip_w8_without_hip_generate_raises_before_a_checkpoint_is_read():
    """The path does not exist: reaching from_pretrained would raise something else than this ValueError"""
    from x2i_amd.infer.inference_multi_turn import MultiTurnConditioner
    from x2i_amd.infer.inference_qwenvl import QwenVLConditioner
    with pytest.raises(ValueError, match="--hip_w8.*--hip_generate"):
        QwenVLConditioner(NO_CHECKPOINT, "cpu", hip_w8=True)
    with pytest.raises(ValueError, match="--hip_w8.*--hip_generate"):
        QwenVLConditioner(NO_CHECKPOINT, "cpu", use_answer=True, hip_head=False, hip_w8=True)
    with pytest.raises(ValueError, match="--hip_w8.*--hip_generate"):
        MultiTurnConditioner(NO_CHECKPOINT, "cpu", hip_w8=True)
    with pytest.raises(ValueError, match="--hip_w8.*--hip_generate"):
        MultiTurnConditioner(NO_CHECKPOINT, "cpu", model=object(), processor=object(), hip_w8=True)


def test_hip_generate_and_decode_step_take_the_option():
    import inspect
    from x2i_amd.handoff import HipGenerate
    from x2i_amd.qwen import Qwen2DecoderStack
    assert inspect.signature(HipGenerate.__init__).parameters["w8"].default is False
    assert inspect.signature(HipGenerate.generate).parameters["w8"].default is None
    assert inspect.signature(Qwen2DecoderStack.decode_step).parameters["w8"].default is False


def test_decode_step_w8_without_a_pack_raises_and_the_pack_hooks_drop_it():
    """Without a device: the refusal comes before the cache is looked at, and the staleness hooks run on a CPU stack with a stand-in pack"""
    from x2i_amd.qwen import Qwen2DecoderStack
    kw = dict(hidden_size=256, num_attention_heads=2, num_key_value_heads=1, intermediate_size=512, num_hidden_layers=1, vocab_size=16, device="cpu")
    m = Qwen2DecoderStack(**kw)
    assert m._w8 is None
    with pytest.raises(ValueError, match=r"pack_w8\(\)"):
        m.decode_step(None, input_ids=torch.zeros((1, 1), dtype=torch.long), w8=True)
    sd = {k: torch.zeros_like(v) for k, v in m.state_dict().items()}
    for hook in (lambda: m.load_state_dict(sd), lambda: m.to("cpu"), lambda: m.bfloat16(), lambda: m.pack_()):
        m._w8 = ["a stand-in pack"]
        hook()
        assert m._w8 is None
    # a width that is no multiple of 16 cannot be packed: a lane's load is 16 weights
    odd = Qwen2DecoderStack(**dict(kw, intermediate_size=520))
    with pytest.raises(ValueError, match="multiples of 16"):
        odd.pack_w8()
