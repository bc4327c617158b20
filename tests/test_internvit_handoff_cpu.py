"""The InternVL2.5 hand-off without a GPU (x2i_amd/handoff.py: find_extract_feature, HipInternVision; x2i_amd/internvit.py; the
`--hip_vision` flag of x2i_amd.infer.inference_internvl) with a stub chat model: install / remove, the wiring, the parameter names and
the refusals."""
import pytest
import torch

from tests import internvit_ref as IR


def _sd(seed=5, cfg=IR.TINY):
    return IR.random_state_dict(cfg, IR.TINY_LLM, seed)


def _tiny(**kw):
    from x2i_amd.internvit import InternVisionTower
    f = dict(IR.TINY)
    dtype = kw.pop("dtype", torch.bfloat16)
    f.update(kw)
    return InternVisionTower(device="cpu", dtype=dtype, **f)


# ---------------------------------------------------------------------------------------------------------------- hand-off
def test_find_extract_feature_and_install_remove_restore_the_instance():
    """install / remove swap `extract_feature` on the instance and restore what was there (nothing, or an earlier instance attribute), on
    an exception too"""
    from x2i_amd import handoff
    model = IR.StubChatModel(_sd())
    assert handoff.find_extract_feature(model) == (model.vision_model, model.mlp1)
    bare = torch.nn.Linear(2, 2)
    with pytest.raises(RuntimeError, match="extract_feature"):
        handoff.find_extract_feature(bare)
    with pytest.raises(RuntimeError, match="extract_feature"):
        handoff.HipInternVision(bare)
    hv = handoff.HipInternVision(model)
    assert hv.vision.graph is True and hv.calls == 0 and "extract_feature" not in model.__dict__
    assert (hv.vision.select_layer, hv.vision.ps_version, hv.vision.downsample_ratio) == (-1, "v2", 0.5)
    with hv:
        assert model.__dict__["extract_feature"] == hv._extract_feature
    assert "extract_feature" not in model.__dict__
    with pytest.raises(KeyError):
        with hv:
            raise KeyError("inside")
    assert "extract_feature" not in model.__dict__
    mine = lambda pixel_values: None
    model.extract_feature = mine
    hv.install().install()
    hv.remove()
    hv.remove()
    assert model.__dict__["extract_feature"] is mine
    del model.extract_feature
    # a model in training mode goes to the original
    x = IR.random_pixels(1, 56, 6).bfloat16()
    with hv:
        model.train()
        out = model.extract_feature(x)
        model.eval()
    assert model.own_calls == 1 and hv.calls == 0 and out.shape == (1, 4, IR.TINY_LLM)
    # what the model says about the tail is read off it
    other = IR.StubChatModel(_sd(), select_layer=-2, ps_version="v1")
    hv2 = handoff.HipInternVision(other, graph=False)
    assert (hv2.vision.select_layer, hv2.vision.n_run, hv2.vision.ps_version, hv2.vision.graph) == (-2, 1, "v1", False)
    other.downsample_ratio = 0.25
    with pytest.raises(ValueError, match="downsample_ratio"):
        handoff.HipInternVision(other)


def test_conditioner_reaches_install_and_the_flag_is_parsed_and_passed(monkeypatch):
    from x2i_amd import handoff
    from x2i_amd.infer import inference_internvl as inf
    from x2i_amd.infer.harness import build_parser
    model = IR.StubChatModel(_sd())
    assert inf.InternVLConditioner(None, "cpu", prefill_only=False, model=model).vision is None and "extract_feature" not in model.__dict__
    cond = inf.InternVLConditioner(None, "cpu", prefill_only=False, model=model, hip_vision=True)       # reaches HipInternVision.install()
    assert isinstance(cond.vision, handoff.HipInternVision) and model.__dict__["extract_feature"] == cond.vision._extract_feature
    cond.vision.remove()
    assert "extract_feature" not in model.__dict__
    with pytest.raises(RuntimeError, match="extract_feature"):
        inf.InternVLConditioner(None, "cpu", prefill_only=False, model=torch.nn.Linear(2, 2), hip_vision=True)
    p = build_parser("internvl")
    assert p.parse_args(["--synthetic"]).hip_vision is False and p.parse_args(["--synthetic", "--hip_vision"]).hip_vision is True
    text = " ".join(p.format_help().split())
    assert "InternVL2.5" in text and "extract_feature" in text and "x2i_amd/internvit.py" in text
    # main hands the flag to the conditioner
    seen = {}

    class Conditioner:
        def __init__(self, path, device, **kw):
            seen.update(kw, path=path)

    class FakeHarness:
        def __init__(self, *a):
            pass

        def run_tasks(self, tasks):
            seen["ran"] = True

    monkeypatch.setattr(inf, "InternVLConditioner", Conditioner)
    monkeypatch.setattr(inf, "Harness", FakeHarness)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    inf.main(["--hip_vision", "--internvl_path", "nowhere"])
    assert seen["hip_vision"] is True and seen["prefill_only"] is True and seen["ran"]
    inf.main(["--internvl_path", "nowhere"])
    assert seen["hip_vision"] is False


# ---------------------------------------------------------------------------------------------------------------- host modules
def test_parameter_names_are_the_references_and_load_strictly():
    from x2i_amd.internvit import InternVisionTower, InternVLVision
    sd = _sd(seed=7)
    vit = {k[len("vision_model."):]: v for k, v in sd.items() if k.startswith("vision_model.")}
    tower = _tiny()
    mine = tower.state_dict()
    assert set(mine) == set(vit) and all(tuple(mine[k].shape) == tuple(vit[k].shape) for k in vit)
    tower.load_state_dict({k: v.bfloat16() for k, v in vit.items()}, strict=True)
    assert all(torch.equal(v.float(), vit[k]) for k, v in tower.state_dict().items())
    with pytest.raises(RuntimeError):
        tower.load_state_dict({k: v.bfloat16() for k, v in vit.items() if k != "encoder.layers.1.ls2"}, strict=True)
    # the Conv2d weight is a view of the zero-padded [hidden, 640] matrix, and the f32 LayerScale copies follow the parameters
    w = tower.embeddings.patch_embedding.weight
    assert w.shape == (128, 3, 14, 14) and w.data_ptr() == tower._pe.data_ptr() and tower._pe.shape == (128, 640) and not bool(tower._pe[:, 588:].any())
    assert torch.equal(tower._pe[:, :588].float(), vit["embeddings.patch_embedding.weight"].reshape(128, 588))
    ls = tower._ls[1][1]
    assert ls.dtype == torch.float32 and torch.equal(ls, vit["encoder.layers.1.ls2"])
    t2 = tower.to(torch.bfloat16)
    assert t2.embeddings.patch_embedding.weight.data_ptr() == t2._pe.data_ptr() and t2._ls[1][1] is not ls and torch.equal(t2._ls[1][1], ls)
    tower.encoder.layers[1].ls2.data.mul_(2)
    assert torch.equal(tower.pack_()._ls[1][1], 2 * ls)
    # the InternViT-6B kind: RMS norms without a bias, q_norm / k_norm, no qkv bias
    big = dict(IR.TINY, norm_type="rms_norm", qk_normalization=True, qkv_bias=False, hidden_size=256, num_attention_heads=2)
    names = set(InternVisionTower(device="cpu", **big).state_dict())
    assert names == set(IR.state_dict_shapes(big)) and "encoder.layers.0.attn.q_norm.weight" in names and "encoder.layers.0.norm1.bias" not in names
    # from_hf copies an instantiated tower; the chat model's names load into InternVLVision
    model = IR.StubChatModel(sd)
    copy = InternVisionTower.from_hf(model.vision_model)
    assert copy.device.type == "cpu" and copy.config.head_dim == 64 and all(torch.equal(v.float(), vit[k]) for k, v in copy.state_dict().items())
    vis = InternVLVision(_tiny(), IR.TINY_LLM)
    assert set(vis.state_dict()) == set(sd)
    vis.load_state_dict({k: v.bfloat16() for k, v in sd.items()}, strict=True)
    assert torch.equal(vis.vision_model._ls[0][0], vit["encoder.layers.0.ls1"])
    from_model = InternVLVision(copy, model.mlp1)
    assert all(torch.equal(v, vis.state_dict()[k]) for k, v in from_model.state_dict().items()) and from_model.llm_hidden_size == IR.TINY_LLM


def test_refusals_name_the_field():
    from x2i_amd.internvit import InternVLVision, layers_to_run
    for bad, msg in ((dict(dtype=torch.float16), "dtype"), (dict(dtype=torch.float32), "dtype"), (dict(hidden_act="gelu_pytorch_tanh"), "hidden_act"),
                     (dict(hidden_act="quick_gelu"), "hidden_act"), (dict(hidden_size=192), "head widths"), (dict(num_attention_heads=4), "head widths"),
                     (dict(norm_type="group_norm"), "norm_type"), (dict(num_hidden_layers=0), "layer"), (dict(patch_size=40), "patch_size")):
        with pytest.raises(ValueError, match=msg):
            _tiny(**bad)
    with pytest.raises(TypeError, match="unknown"):
        _tiny(depth=2)
    with pytest.raises(ValueError, match="bf16"):
        _tiny().float()
    with pytest.raises(ValueError, match="eval-only"):
        _tiny().train()
    assert _tiny(num_attention_heads=1).config.head_dim == 128
    tower = _tiny()
    for bad, msg in ((dict(downsample_ratio=0.25), "downsample_ratio"), (dict(ps_version="v3"), "ps_version"), (dict(select_layer=-4), "select_layer"),
                     (dict(select_layer=3), "select_layer")):
        with pytest.raises(ValueError, match=msg):
            InternVLVision(tower, IR.TINY_LLM, **bad)
    assert [layers_to_run(s, 24) for s in (-1, -2, -25, 0, 24)] == [24, 23, 0, 0, 24]
    vis = InternVLVision(tower, IR.TINY_LLM)
    with pytest.raises(ValueError, match="grid must be even"):
        vis.plan(1, 3)
    with pytest.raises(ValueError, match="grid must be square"):
        vis(torch.zeros((1, 3, 28, 56), dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="grid must be even"):
        vis(torch.zeros((1, 3, 42, 42), dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="pixel_values"):
        vis(torch.zeros((1, 3, 50, 56), dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="runs on the GPU only"):
        vis(torch.zeros((1, 3, 56, 56), dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="pixel_values only"):
        tower(pixel_values=torch.zeros((1, 3, 56, 56)), output_hidden_states=True)
