"""The InternVL2.5 vision path without a GPU: the restatement of tests/internvit_ref.py against what the reference's own modules recorded
(tests/golden/internvit_tiny.safetensors, written by tests/golden/make_internvit_golden.py), the planted faults against the checker the
GPU test uses, and the boundary of include/x2i_internvit.h (the binding's prototypes, argument validation through ctypes)."""
import ctypes as C
import os

import pytest
import torch
from safetensors.torch import load_file

from tests import internvit_ref as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESTATEMENT_BOUND = 1e-10
F64 = torch.float64


@pytest.fixture(scope="module")
def fx():
    t = load_file(os.path.join(ROOT, "tests", "golden", "internvit_tiny.safetensors"))
    return t, IR.unpack_state_dict(t)


@pytest.fixture(scope="module")
def truth(fx):
    """float64 restatement of extract_feature on the fixture, computed once"""
    t, sd = fx
    return IR.extract_feature(sd, t["x"].float(), IR.TINY, F64)


# ---------------------------------------------------------------------------------------------------------------- restatement
def test_fixture_is_data_of_the_stated_configuration(fx):
    t, sd = fx
    assert set(sd) == set(IR.state_dict_shapes(IR.TINY, IR.TINY_LLM))
    assert all(tuple(sd[k].shape) == s for k, s in IR.state_dict_shapes(IR.TINY, IR.TINY_LLM).items())
    assert all(torch.equal(v.bfloat16().float(), v) for v in sd.values())                 # bf16 values, so the bf16 modules load them exactly
    assert tuple(t["x"].shape) == (2, 3, 56, 56) and tuple(t["last_hidden_state"].shape) == (2, 17, 128)
    assert tuple(t["extract_feature"].shape) == (2, 4, 192) and t["extract_feature"].dtype == F64
    ls = torch.cat([sd["vision_model.encoder.layers.%d.ls%d" % (i, j)] for i in range(2) for j in (1, 2)])
    assert float(ls.std()) > 0.02                                                          # not 0.1 everywhere
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "internvit_tiny.safetensors")) < os.path.getsize(
        os.path.join(ROOT, "tests", "golden", "resampler_tiny.safetensors"))


def test_float64_restatement_meets_the_recorded_outputs(fx, truth):
    t, sd = fx
    x = t["x"].float()
    last = IR.tower(sd, x, IR.TINY, F64, prefix="vision_model.")
    assert IR.rel_l2(last, t["last_hidden_state"]) < RESTATEMENT_BOUND
    assert IR.rel_l2(truth, t["extract_feature"]) < RESTATEMENT_BOUND
    # select_layer -2 is hidden_states[-2]: one layer fewer, and another tensor
    m2 = IR.tower(sd, x, IR.TINY, F64, select_layer=-2, prefix="vision_model.")
    assert IR.rel_l2(m2, t["hidden_m2"]) < RESTATEMENT_BOUND and IR.rel_l2(m2, t["last_hidden_state"]) > 1e-2
    assert torch.equal(IR.tower(sd, x, IR.TINY, F64, select_layer=1, prefix="vision_model."), m2)
    assert torch.equal(IR.tower(sd, x, IR.TINY, F64, select_layer=2, prefix="vision_model."), last)


def test_position_table_at_another_grid_is_the_recorded_call(fx):
    t, sd = fx
    pos = sd["vision_model.embeddings.position_embedding"].double()
    got = IR.position_table(pos, 4, 6, 6)
    assert got.shape == (1, 37, 128) and torch.equal(got[:, :1], pos[:, :1])
    assert IR.rel_l2(got[:, 1:], t["pos_6x6"]) < RESTATEMENT_BOUND
    assert torch.equal(IR.position_table(pos, 4, 4, 4), pos)                               # the identity at the native grid
    last6 = IR.tower(sd, t["x6"].float(), IR.TINY, F64, prefix="vision_model.")
    assert IR.rel_l2(last6, t["last_hidden_state_6x6"]) < RESTATEMENT_BOUND
    # the module's table is the same call on the bf16 parameter
    from x2i_amd.internvit import InternVisionTower
    tower = InternVisionTower(device="cpu", **IR.TINY)
    tower.load_state_dict({k[len("vision_model."):]: v.bfloat16() for k, v in sd.items() if k.startswith("vision_model.")}, strict=True)
    assert torch.equal(tower.position_table(6, 6), IR.position_table(pos.bfloat16(), 4, 6, 6)[0])
    assert torch.equal(tower.position_table(4, 4), pos.bfloat16()[0]) and tower.position_table(6, 6) is tower.position_table(6, 6)


def test_ps_version_v1_is_the_transposed_v2():
    g, D = 6, 8
    tokens = torch.arange(2 * g * g * D, dtype=F64).reshape(2, g * g, D)
    v2, v1 = IR.shuffle_gather(tokens, g), IR.shuffle_gather(tokens, g, v1=True)
    assert v2.shape == v1.shape == (2, 9, 4 * D) and not torch.equal(v1, v2)
    assert torch.equal(v1.reshape(2, 3, 3, 4 * D), v2.reshape(2, 3, 3, 4 * D).transpose(1, 2))
    # row t = r' g/2 + q' of v2, chunk (dr, dq): token (2r' + dr, 2q' + dq)
    for rr, qq, dr, dq in ((0, 0, 0, 0), (1, 2, 0, 1), (2, 1, 1, 0), (2, 2, 1, 1)):
        k = 2 * dr + dq
        assert torch.equal(v2[:, rr * 3 + qq, k * D:(k + 1) * D], tokens[:, (2 * rr + dr) * g + 2 * qq + dq])


def test_sdpa_and_naive_attention_agree_in_float64(fx, truth):
    t, sd = fx
    assert IR.rel_l2(IR.extract_feature(sd, t["x"].float(), IR.TINY, F64, attn="sdpa"), truth) < RESTATEMENT_BOUND


# ---------------------------------------------------------------------------------------------------------------- planted faults
def test_the_checker_passes_the_bf16_restatement(fx):
    t, sd = fx
    run = lambda w, x: IR.extract_feature(w, x, IR.TINY, torch.bfloat16, attn="sdpa")
    pairs = IR.check_extract_feature("bf16 restatement under sdpa", run, sd, t["x"].float(), IR.TINY)
    assert len(pairs) == 2 and all(e > 1e-4 for _, e, _ in pairs)


@pytest.mark.parametrize("fault", IR.FAULTS)
def test_planted_faults_are_rejected_by_the_checker_of_the_gpu_test(fx, fault):
    """each fault runs in float64 -- nothing but the fault separates it from the judge -- and check_extract_feature, the checker of
    tests/test_internvit_gpu.py, must refuse it"""
    t, sd = fx
    run = lambda w, x: IR.extract_feature(w, x, IR.TINY, F64, fault=fault)
    with pytest.raises(AssertionError, match="1.5 x bf16 restatement"):
        IR.check_extract_feature(fault, run, sd, t["x"].float(), IR.TINY)


def test_gelu_form_is_invisible_without_the_activation_probe(fx, truth):
    """why the checker has a second weight set: on the test weights the tanh form is an order of magnitude below the bf16 floor"""
    t, sd = fx
    x = t["x"].float()
    e_tanh = IR.rel_l2(IR.extract_feature(sd, x, IR.TINY, F64, fault="gelu_tanh"), truth)
    e_bf16 = IR.rel_l2(IR.extract_feature(sd, x, IR.TINY, torch.bfloat16), truth)
    assert e_tanh < 0.2 * e_bf16
    probe = IR.activation_probe(sd)
    ref = IR.extract_feature(probe, x, IR.TINY, F64)
    # on the probe weights it is twice over what the criterion's factor of 1.5 lets pass (measured: 6.4e-2 against a floor of 1.4e-2)
    assert IR.rel_l2(IR.extract_feature(probe, x, IR.TINY, F64, fault="gelu_tanh"), ref) > 3 * IR.rel_l2(IR.extract_feature(probe, x, IR.TINY, torch.bfloat16), ref)
    assert all(torch.equal(v.bfloat16().float(), v) for v in probe.values())


# ---------------------------------------------------------------------------------------------------------------- boundary
def test_entry_points_validate_their_arguments_without_a_gpu():
    from x2i_amd import internvit_ops
    lib = internvit_ops.load()
    fake = C.c_void_p(0x1000)  # never dereferenced: validation fails first
    err = lambda: lib.x2i_last_error()
    rows = lambda **kw: lib.x2i_internvit_patch_rows_bf16(*[kw.get(k, d) for k, d in (
        ("img", fake), ("ibs", 3 * 28 * 42), ("ics", 28 * 42), ("ild", 42), ("Xp", fake), ("ldx", 640), ("B", 2), ("gh", 2), ("gw", 3), ("P", 14),
        ("Kp", 640), ("st", None))])
    assert rows(P=0) < 0 and b"P=0" in err()
    assert rows(P=33, Kp=3272, ldx=3272, ild=99, ics=66 * 99, ibs=3 * 66 * 99) < 0 and b"P=33" in err()
    assert rows(B=0) < 0 and rows(gh=0) < 0 and rows(gw=0) < 0
    assert rows(B=70000, gh=1000, gw=1000, ild=14000, ics=14000 * 14000, ibs=3 * 14000 * 14000) < 0 and b"2^31" in err()
    assert rows(Kp=584, ldx=584) < 0 and b"Kp=584" in err()     # < 3 * P * P
    assert rows(Kp=636) < 0 and b"Kp=636" in err()             # not a multiple of 8
    assert rows(ldx=632) < 0 and b"ldx" in err()               # < Kp
    assert rows(ldx=644) < 0 and b"ldx" in err()
    assert rows(ild=41) < 0 and b"img_ld" in err()             # < gw * P
    assert rows(ics=28 * 42 - 1) < 0 and b"img_chan_stride" in err()
    assert rows(ibs=3 * 28 * 42 - 1) < 0 and b"img_batch_stride" in err()
    assert rows(Xp=C.c_void_p(0x1008)) < 0 and b"aligned" in err()
    assert rows(img=C.c_void_p(0x1001)) < 0 and b"aligned" in err()
    for k in ("img", "Xp"):
        assert rows(**{k: None}) < 0 and b"null" in err()
    emb = lambda **kw: lib.x2i_internvit_embed_bf16(*[kw.get(k, d) for k, d in (
        ("X", fake), ("cls", fake), ("pos", fake), ("B", 2), ("L", 6), ("D", 64), ("st", None))])
    assert emb(D=60) < 0 and b"D=60" in err()
    assert emb(D=0) < 0 and emb(B=0) < 0 and emb(L=0) < 0
    for k in ("X", "cls", "pos"):
        assert emb(**{k: None}) < 0 and b"null" in err()
        assert emb(**{k: C.c_void_p(0x1008)}) < 0 and b"aligned" in err()
    sln = lambda **kw: lib.x2i_internvit_shuffle_ln_bf16(*[kw.get(k, d) for k, d in (
        ("X", fake), ("xbs", 17 * 64), ("ldx", 64), ("Y", fake), ("ldy", 256), ("w", fake), ("b", fake), ("B", 2), ("g", 4), ("D", 64),
        ("eps", 1e-5), ("v1", 0), ("st", None))])
    assert sln(g=3, xbs=10 * 64) < 0 and b"g=3" in err()
    assert sln(g=0) < 0 and sln(g=-2) < 0 and sln(B=0) < 0
    assert sln(D=60, ldx=64) < 0 and b"D=60" in err()
    assert sln(D=1032, ldx=1032, xbs=17 * 1032, ldy=4128) < 0 and b"D=1032" in err()      # 4 * D beyond the row kernel's 4096
    assert sln(ldx=56) < 0 and b"ldx" in err()
    assert sln(ldx=68, xbs=17 * 68) < 0
    assert sln(xbs=17 * 64 - 8) < 0 and b"x_batch_stride" in err()
    assert sln(xbs=17 * 64 + 4) < 0
    assert sln(ldy=248) < 0 and sln(ldy=260) < 0 and b"ldy" in err()
    for k in ("X", "Y", "w", "b"):
        assert sln(**{k: None}) < 0 and b"null" in err()
        assert sln(**{k: C.c_void_p(0x1008)}) < 0 and b"aligned" in err()
