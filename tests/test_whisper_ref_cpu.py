"""The float64 reference of the MiniCPM-o Whisper audio tower (tests/whisper_ref.py) against `transformers`' own Whisper submodules, and the
host arithmetic of x2i_amd/whisper.py -- key ranges, token counts, the pooling order -- against the model's formulas.  No GPU."""
import pytest
import torch

from tests import whisper_ref as WR


@pytest.fixture(scope="module")
def tiny():
    cfg, apm, proj = WR.library_tower(128, 2, 256, 2, 150, 96)
    sd = WR.random_state_dict(apm, proj, seed=5)
    WR.load_state_dict_into(apm, proj, sd)
    return cfg, apm.double(), proj.double(), sd


@pytest.mark.parametrize("T,lens,chunk_length,k", [(7, [7], 1.0, 2), (260, [260, 90], 1.0, 2), (61, [61, 23], 0.1, 5), (24, [24, 9], -1, 1)])
def test_float64_restatement_equals_the_library_composition_in_float64(tiny, T, lens, chunk_length, k):
    cfg, apm, proj, sd = tiny
    mel = WR.random_mel(len(lens), T, lens, seed=T)
    want = WR.library_forward(apm, proj, mel.double(), lens, chunk_length, k)
    got = WR.tower_reference(sd, mel, lens, num_heads=2, chunk_length=chunk_length, k=k)
    assert [t.shape for t in got] == [t.shape for t in want] == [(n, 96) for n in WR.token_counts(lens, k)]
    for a, b in zip(got, want):
        assert WR.rel_l2(a, b) < 1e-10


@pytest.mark.parametrize("S,C,n", [(4, 50, 7), (130, 50, 260), (130, 50, 90), (130, 5, 200), (7, 3, 2)])
def test_key_ranges_equal_the_models_boolean_mask_row_by_row(S, C, n):
    from x2i_amd.whisper import key_ranges
    hi = key_ranges([n], S, C)
    assert hi.dtype == torch.int32 and hi.shape == (1, S)
    dead = WR.masked_keys([n], S, C / 50)
    assert int(C / 50 * 50) == C
    for i in range(S):
        want = ~dead[0, i]
        assert bool(want[:int(hi[0, i])].all()) and not bool(want[int(hi[0, i]):].any()), (i, int(hi[0, i]))
        assert int(hi[0, i]) == min(n, S, (i // C + 1) * C) >= 1


@pytest.mark.parametrize("chunk_length", [-1, 0])
def test_no_chunking_leaves_the_padding_alone(chunk_length):
    from x2i_amd.whisper import key_ranges
    hi = key_ranges([260, 90, 1], 130, int(chunk_length * 50))
    dead = WR.masked_keys([260, 90, 1], 130, chunk_length)
    assert hi.tolist() == [[130] * 130, [90] * 130, [1] * 130]
    assert torch.equal((~dead).sum(-1).to(torch.int32), hi)


def test_token_counts_equal_the_models_formula():
    from x2i_amd.whisper import conv_rows, token_counts
    from x2i_amd.whisper_ops import pooled_rows
    for k in (1, 2, 5):
        lens = list(range(1, 13))
        after_cnn = [(n - 1) // 2 + 1 for n in lens]
        want = [(s - k) // k + 1 for s in after_cnn]        # _get_feat_extract_output_lengths, Python's floor division as torch's
        assert token_counts(lens, k) == [max(v, 0) for v in want] == [max(v, 0) for v in WR.token_counts(lens, k)]
        assert [conv_rows(n) for n in lens] == after_cnn
        for s in after_cnn:
            x = torch.zeros((1, 3, s))
            assert pooled_rows(s, k) == (torch.nn.functional.avg_pool1d(x, k, k).shape[-1] if s >= k else 0)
    # the conv's own arithmetic
    for T in range(1, 13):
        y = torch.nn.Conv1d(2, 2, 3, stride=2, padding=1)(torch.nn.Conv1d(2, 2, 3, padding=1)(torch.zeros((1, 2, T))))
        assert y.shape[-1] == conv_rows(T)


def test_pool_then_linear2_equals_linear2_then_pool_in_float64(tiny):
    cfg, apm, proj, sd = tiny
    lens = [61, 30]
    mel = WR.random_mel(2, 61, lens, seed=9)
    for k in (2, 5):
        a = WR.tower_reference(sd, mel, lens, num_heads=2, chunk_length=1.0, k=k)
        b = WR.tower_reference(sd, mel, lens, num_heads=2, chunk_length=1.0, k=k, pool_first=True)
        for x, y in zip(a, b):
            assert x.shape == y.shape and WR.rel_l2(x, y) < 1e-12


def test_reference_rows_helpers():
    mel = torch.arange(2 * 3 * 5, dtype=torch.float32).reshape(2, 3, 5) + 1
    rows = WR.mel_rows(mel, 16)
    assert rows.shape == (10, 16) and not bool(rows[:, 9:].any())
    for b in range(2):
        for t in range(5):
            for ci in range(3):
                for k in range(3):
                    want = mel[b, ci, t + k - 1] if 0 <= t + k - 1 < 5 else 0.0
                    assert rows[b * 5 + t, ci * 3 + k] == want
    x = torch.randn((2, 11, 8)).bfloat16()
    y = WR.pool_rows_f32(x, 5)
    assert y.shape == (2, 2, 8) and y.dtype == torch.bfloat16
    assert torch.equal(y[1, 1], ((((x[1, 5].float() + x[1, 6].float()) + x[1, 7].float()) + x[1, 8].float() + x[1, 9].float()) / 5).bfloat16())
