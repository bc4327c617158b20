"""The MiniCPM-o Whisper audio tower on the HIP path (include/x2i_whisper.h, x2i_amd/whisper.py, handoff.HipAudio) on the GPU: the two row
kernels bit for bit against torch, the attention in the regime the tower runs it in (heads of 64, chunked key ranges) against the float64
checker of tests/qwen_vision_ref.py, and the tower with its tail and the hand-off against float64 and against the same computation composed
from `transformers`' Whisper submodules in bf16 on the same GPU (no worse than 1.5 x the library's own error)."""
import pytest
import torch

from tests import qwen_vision_ref as VR
from tests import whisper_ref as WR
from tests.test_t5_gpu import assert_stack_criterion, is_sentinel, poisoned  # (helpers; its tests are not re-collected here)

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def whisper_ops():
    from x2i_amd import whisper_ops as o
    o.load()
    return o


# ---------------------------------------------------------------------------------------------------------------- mel rows
@pytest.mark.parametrize("B,Cin,T", [(1, 80, 1), (2, 80, 7), (1, 80, 260), (2, 8, 131)])
def test_mel_rows_is_the_torch_unfold(whisper_ops, B, Cin, T):
    """mel that is a window of a wider tensor (a row stride beyond T, a start that is only 2-byte aligned), an output wider than Kp and
    longer than B * T: the footprint is rows < B * T, columns < Kp, and the tail columns 3 Cin .. Kp-1 are zero"""
    g = torch.Generator().manual_seed(100 * T + B)
    wide = torch.randn((B, Cin, T + 10), generator=g).bfloat16().to(DEV)
    mel = wide[:, :, 3:3 + T]
    assert mel.data_ptr() % 4 == 2 and (T == 1 or not mel.is_contiguous())
    want = torch.nn.functional.pad(mel, (1, 1)).unfold(2, 3, 1).permute(0, 2, 1, 3).reshape(B * T, 3 * Cin)
    assert torch.equal(want, WR.mel_rows(mel))
    for Kp in ((3 * Cin + 7) // 8 * 8, 256):
        buf = poisoned(B * T + 2, Kp + 16)
        whisper_ops.mel_rows(mel, buf, Kp)
        assert torch.equal(buf[:B * T, :3 * Cin], want)
        assert not bool(buf[:B * T, 3 * Cin:Kp].view(torch.int16).any())
        assert bool(is_sentinel(buf[B * T:]).all()) and bool(is_sentinel(buf[:, Kp:]).all())
        again = poisoned(B * T + 2, Kp + 16)
        whisper_ops.mel_rows(mel.contiguous(), again, Kp)
        assert torch.equal(again, buf)              # the contiguous copy gives the same rows


def test_mel_rows_refusals(whisper_ops):
    from x2i_amd._lib import X2IError
    mel = torch.zeros((2, 80, 7), dtype=torch.bfloat16, device=DEV)
    out = poisoned(14, 256)
    for bad in (dict(Kp=232), dict(Kp=244), dict(ldx=248), dict(ldx=260), dict(mel=mel.float()), dict(mel=mel.transpose(1, 2)), dict(mel=mel[:, :, ::2]),
                dict(mel=mel[0]), dict(out=poisoned(13, 256)), dict(out=poisoned(14, 248))):
        kw = dict(mel=mel, out=out, Kp=256, ldx=None)
        kw.update(bad)
        with pytest.raises(X2IError):
            whisper_ops.mel_rows(kw["mel"], kw["out"], kw["Kp"], ldx=kw["ldx"])
    assert bool(is_sentinel(out).all())         # refused before any launch


# ---------------------------------------------------------------------------------------------------------------- pool rows
@pytest.mark.parametrize("B,S,D,k", [(1, 1, 8, 1), (2, 7, 144, 2), (1, 131, 1024, 2), (1, 11, 64, 5)])
def test_pool_rows_is_the_f32_formula(whisper_ops, B, S, D, k):
    """bit-equal to bf16(sum in index order / k); rows and columns beyond the footprint untouched; the rows of X beyond k * n_out, which are
    NaN here, leave no trace; the strides honoured"""
    g = torch.Generator().manual_seed(S * 10 + k)
    n = (S - k) // k + 1
    x = torch.randn((B, S, D), generator=g).bfloat16().to(DEV)
    want = WR.pool_rows_f32(x, k)
    assert want.shape == (B, n, D)
    xw = torch.full((B, S + 1, D + 8), NAN, dtype=torch.bfloat16, device=DEV)
    xw[:, :k * n, :D] = x[:, :k * n]
    buf = poisoned(B, n + 1, D + 16)
    whisper_ops.pool_rows(xw, buf, B, S, D, k, x_batch_stride=(S + 1) * (D + 8), y_batch_stride=(n + 1) * (D + 16))
    assert torch.equal(buf[:, :n, :D], want)
    assert bool(is_sentinel(buf[:, n:]).all()) and bool(is_sentinel(buf[:, :, D:]).all())
    tight = torch.empty((B, n, D), dtype=torch.bfloat16, device=DEV)
    whisper_ops.pool_rows(x, tight, B, S, D, k)
    assert torch.equal(tight, want)
    if k == 2:      # (a power of two: the f32 division is exact, so torch's f32 pooling rounds the same value)
        assert torch.equal(torch.nn.functional.avg_pool1d(x.float().transpose(1, 2), k, k).transpose(1, 2).bfloat16(), want)


def test_pool_rows_refusals(whisper_ops):
    from x2i_amd._lib import X2IError
    x = torch.zeros((2, 7, 16), dtype=torch.bfloat16, device=DEV)
    out = poisoned(2, 3, 16)
    for bad in (dict(k=0), dict(k=9), dict(S=1), dict(D=12), dict(ldx=8), dict(ldy=8), dict(ldx=20), dict(x_batch_stride=7 * 16 - 8), dict(y_batch_stride=2 * 16),
                dict(x=x.float()), dict(out=poisoned(2, 2, 16)), dict(B=3)):
        kw = dict(x=x, out=out, B=2, S=7, D=16, k=2, ldx=None, ldy=None, x_batch_stride=None, y_batch_stride=None)
        kw.update(bad)
        with pytest.raises(X2IError):
            whisper_ops.pool_rows(kw["x"], kw["out"], kw["B"], kw["S"], kw["D"], kw["k"], ldx=kw["ldx"], ldy=kw["ldy"],
                                  x_batch_stride=kw["x_batch_stride"], y_batch_stride=kw["y_batch_stride"])
    assert bool(is_sentinel(out).all())


# ---------------------------------------------------------------------------------------------------------------- attention, the tower's regime
# (B, H, S, C, the mel lengths): the regime WhisperAudioTower runs x2i_vit_attention_bf16 in.  Heads of 64, scale 64 ** -0.5, row i of
# sample b sees the keys [0, min(len_b, S, (i // C + 1) * C)): the ranges cross a 64-key tile, a 128-row block and -- C = 50, C = 5 -- end
# inside a tile.  Worst tile measured on the MI355X, in this order: 1.75e-3, 3.02e-3, 2.22e-3, 2.25e-3 (bound TOL_O = 5e-3;
# profiles/whisper_gputest.log)
CHUNKED_CASES = [(1, 1, 4, 50, [7]), (1, 2, 130, 50, [260]), (2, 2, 130, 50, [260, 90]), (1, 1, 300, 5, [600])]


@pytest.mark.parametrize("B,H,S,C,lens", CHUNKED_CASES)
def test_attention_with_chunked_ranges_vs_fp64_per_tile(B, H, S, C, lens):
    from x2i_amd import vit_ops
    from x2i_amd.whisper import key_ranges
    Spad = vit_ops.pad64(S)
    Q, K, V = VR.attention_inputs(B, H, S, 64, seed=1000 * S + H + C, device=DEV)
    hi_cpu = key_ranges(lens, S, C)
    lo, hi = torch.zeros((B, S), dtype=torch.int32, device=DEV), hi_cpu.to(DEV)
    buf = poisoned(B, S, H * 64)
    vit_ops.attention(Q, K, V.transpose(-1, -2).contiguous(), buf, B, H, S, Spad, 64, 0.125, H * 64, S * H * 64, lo, hi)
    O = buf.reshape(B, S, H, 64).permute(0, 2, 1, 3)
    ref = VR.attention_reference(Q, K, V, S, 64, 0.125, lo.tolist(), hi_cpu.tolist())
    name = "vit_attention, heads of 64, chunks of %d: B=%d H=%d S=%d mel lengths %s" % (C, B, H, S, lens)
    worst = VR.check_attention(name, O, ref, VR.TOL_O)
    print("%s: worst tile rel-L2 %.3e (bound %.1e)" % (name, worst, VR.TOL_O))
    assert not bool(is_sentinel(buf).any())
    # the chunk edges matter: the reference without them is another result
    if S >= 100:
        full = key_ranges(lens, S, 0)
        assert VR.rel_l2(VR.attention_reference(Q, K, V, S, 64, 0.125, lo.tolist(), full.tolist()), ref) > 1e-3


# ---------------------------------------------------------------------------------------------------------------- tower plus tail
# (d_model, heads, ffn, layers, E, T, mel lengths, C, k): a tiny tower on seven frames; a padded batch where the mel length 90 meets post-conv
# indices (sample 1 sees 90 keys though 45 of its rows are real); one full-width layer (1024, 16 heads of 64, 4096, E = 3584) on 600 frames.
# Measured on the MI355X, HIP / library bf16 against float64: 5.30e-3 / 8.49e-3, 4.14e-3 / 5.09e-3, 4.27e-3 / 5.31e-3 (ratio 0.62, 0.81, 0.80;
# the criterion allows 1.5; profiles/whisper_gputest.log; the library's last figure was 5.62e-3 in another run, the HIP figures did not move)
TOWER_CASES = [(128, 2, 512, 2, 192, 7, [7], 50, 2), (128, 2, 512, 2, 192, 260, [260, 90], 50, 2), (1024, 16, 4096, 1, 3584, 600, [600], 50, 2)]


@pytest.mark.parametrize("D,heads,ffn,layers,E,T,lens,C,k", TOWER_CASES)
def test_tower_and_tail_vs_fp64_and_the_librarys_bf16(D, heads, ffn, layers, E, T, lens, C, k):
    from x2i_amd.whisper import WhisperAudioTower
    cfg, apm, proj = WR.library_tower(D, heads, ffn, layers, 1500, E)
    sd = WR.random_state_dict(apm, proj, seed=D + T)
    WR.load_state_dict_into(apm, proj, sd)
    hip = WhisperAudioTower.from_hf(apm, proj, k).to(DEV)      # the views follow their packed storage to the GPU; conv2's copy is made again there
    assert hip.apm.conv1.weight.data_ptr() == hip._fused["c1"].data_ptr() and hip._conv2.device.type == "cuda"
    B = len(lens)
    mel = WR.random_mel(B, T, lens, seed=T)
    x = mel.bfloat16().to(DEV)
    counts = WR.token_counts(lens, k)
    out, got_counts = hip(x, feature_lens=lens, chunk_frames=C)
    assert got_counts == counts and out.shape == (B, max(counts), E) and out.dtype == torch.bfloat16
    first = out.clone()
    assert bool(torch.isfinite(first).all())
    # a second call with the same plan is bit-identical, and a planned forward only enqueues
    plan = hip.plan(lens, T, C)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = hip(x, plan=plan)[0]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(again, first)
    # a sample whose length is the batch's T is bit-identical alone and inside the batch (a shorter one is not: the conv sees other padding
    # and the keys other rows)
    if B > 1:
        for b, n in enumerate(lens):
            if n == T:
                alone, c1 = hip(x[b:b + 1], feature_lens=[n], chunk_frames=C)
                assert c1 == [counts[b]] and torch.equal(alone[0, :counts[b]], first[b, :counts[b]]), "sample %d of %s" % (b, lens)
    ref = torch.cat(WR.tower_reference(sd, mel, lens, num_heads=heads, chunk_length=C / 50, k=k))
    lib16 = torch.cat(WR.library_forward(apm.to(device=DEV, dtype=torch.bfloat16), proj.to(device=DEV, dtype=torch.bfloat16), mel, lens, C / 50, k))
    mine = torch.cat([first[b, :n] for b, n in enumerate(counts)])
    e_hip, e_lib = WR.rel_l2(mine, ref), WR.rel_l2(lib16, ref)
    print("WhisperAudioTower d_model=%d heads=%d ffn=%d layers=%d E=%d T=%d lens %s C=%d k=%d: rel-L2 against float64: HIP %.3e, transformers bf16 on "
          "the GPU %.3e (ratio %.2f)" % (D, heads, ffn, layers, E, T, lens, C, k, e_hip, e_lib, e_hip / e_lib))
    assert_stack_criterion(e_hip, e_lib)


def test_tower_defaults_and_plan_mismatch():
    from x2i_amd.whisper import WhisperAudioTower
    hip = WhisperAudioTower(d_model=128, encoder_attention_heads=2, encoder_ffn_dim=256, encoder_layers=1, max_source_positions=64, embed_dim=96,
                            pool_step=2, device=DEV).init_random_(3)
    x = WR.random_mel(2, 9, [9, 9], seed=4).to(DEV)
    want, counts = hip(x, feature_lens=torch.tensor([9, 9]))
    assert counts == [2, 2] and want.shape == (2, 2, 96)
    assert torch.equal(hip(x)[0], want)                          # no lengths: all T
    assert torch.equal(hip(x.bfloat16().transpose(1, 2).contiguous().transpose(1, 2))[0], want)      # any strides
    assert not torch.equal(hip(x, chunk_frames=2)[0], want)      # the chunk mask counts
    one, c = hip(x[:, :, :1])
    assert one.shape == (2, 0, 96) and c == [0, 0]              # one token and nothing to pool
    with pytest.raises(ValueError, match="plan is for"):
        hip(x[:1], plan=hip.plan([9, 9], 9))
    with pytest.raises(ValueError, match="embed_positions"):
        hip(torch.zeros((1, 80, 129), device=DEV))


# ---------------------------------------------------------------------------------------------------------------- hand-off
def test_hip_audio_replaces_get_audio_embedding_and_restores_it():
    from x2i_amd.handoff import HipAudio
    cfg, apm, proj = WR.library_tower(128, 2, 256, 2, 150, 96)
    WR.load_state_dict_into(apm, proj, WR.random_state_dict(apm, proj, seed=21))
    model = WR.StandInModel(apm.to(device=DEV, dtype=torch.bfloat16), proj.to(device=DEV, dtype=torch.bfloat16), 2)
    lens = [61, 30, 44]
    mel = WR.random_mel(3, 61, lens, seed=22).bfloat16().to(DEV)
    data = {"audio_features": mel, "audio_feature_lens": [torch.tensor([61, 30]), torch.tensor([44])]}
    theirs = model.get_audio_embedding(data, chunk_length=0.2)   # chunks of ten tokens among S = 31
    assert model.original_calls == 1
    ha = HipAudio(model)
    with ha:
        assert "get_audio_embedding" in model.__dict__
        got = model.get_audio_embedding(data, chunk_length=0.2)
        assert ha.calls == 1 and model.original_calls == 1
        assert [len(g) for g in got] == [len(t) for t in theirs] == [2, 1]
        for g, t in zip(got, theirs):
            for a, b in zip(g, t):
                assert a.shape == b.shape and a.dtype == torch.bfloat16 and WR.rel_l2(a, b) < 3e-2
        assert [tuple(a.shape) for g in got for a in g] == [(15, 96), (7, 96), (11, 96)]
        full = model.get_audio_embedding(data)                   # chunk_length = -1: no chunking, another result
        assert ha.calls == 2 and WR.rel_l2(full[0][0], got[0][0]) > 1e-3
        assert model.get_audio_embedding({"audio_features": [], "audio_feature_lens": []}) == [] and ha.calls == 2
    assert "get_audio_embedding" not in model.__dict__ and model.original_calls == 1
    assert len(model.get_audio_embedding(data, chunk_length=0.2)) == 2 and model.original_calls == 2 and ha.calls == 2
    with pytest.raises(KeyError):
        with ha:
            raise KeyError("inside")
    assert "get_audio_embedding" not in model.__dict__
