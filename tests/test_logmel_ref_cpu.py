"""The float64 reference of the log-mel front end (tests/logmel_ref.py) against transformers' WhisperFeatureExtractor, called as the
MiniCPM-o processor calls it, on six signals; the two frame counts L and A; and the case in which a dropped frame holds the maximum."""
import functools

import numpy as np
import pytest

from tests import logmel_ref as LR

N_MAX = 480000
NAMES = ("noise", "tone", "clip", "burst", "chirp", "zeros")


@functools.lru_cache(maxsize=None)
def _extractor():
    from transformers import WhisperFeatureExtractor
    return WhisperFeatureExtractor()


@functools.lru_cache(maxsize=None)
def _case(name):
    x = LR.six_signals()[name]
    got = _extractor()([x], sampling_rate=16000, return_attention_mask=True, padding="max_length", return_tensors="pt")
    lg, out = LR.ref64(x, N_MAX, LR.mel_filters(80))
    return x, got["input_features"][0].numpy(), int(got["attention_mask"][0].sum()), lg, out


@pytest.mark.parametrize("name", NAMES)
def test_float64_reference_matches_the_feature_extractor(name):
    x, feat, mask_len, lg, out = _case(name)
    assert feat.shape == out.shape == (80, 3000)
    err = float(np.abs(feat.astype(np.float64) - out).max())
    rest = float(np.abs(LR.restate32(x, N_MAX, LR.mel_filters(80)).astype(np.float64) - out).max())
    print("%s: extractor vs float64 reference %.3g, float32 restatement vs float64 reference %.3g" % (name, err, rest))
    assert err <= 1e-4
    assert LR.kept_frames(len(x), N_MAX) == mask_len
    if name == "zeros":
        assert (out == -1.5).all() and (feat == -1.5).all() and (lg == -10.0).all()


@pytest.mark.parametrize("name", [n for n in NAMES if n != "zeros"])
def test_seen_frames_is_the_count_of_frames_that_differ_from_the_floor(name):
    """A by brute force, twice: the frames that hold a non-zero sample, and the frames of the reference that are not exactly -10.  The
    second count can only be smaller, and is for "burst": its last seen frame holds 40 samples of 1e-5 under the window's first 40 weights,
    a mel power below the floor 1e-10 -- a frame that is -10 although it sees a sample, which is why no frame below A may be skipped."""
    x, _, _, lg, _ = _case(name)
    A = LR.seen_frames(len(x), N_MAX)
    sees = np.nonzero((LR.frames64(x, N_MAX) != 0.0).any(axis=1))[0]
    assert int(sees[-1]) + 1 == A >= LR.kept_frames(len(x), N_MAX)
    live = np.nonzero((lg != -10.0).any(axis=0))[0]
    assert int(live[-1]) + 1 == (A - 1 if name == "burst" else A)


def test_frame_counts():
    assert [LR.kept_frames(n, N_MAX) for n in (1, 159, 160, 161, 960, 1000, 479999, 480000)] == [1, 1, 1, 2, 6, 7, 3000, 3000]
    assert [LR.seen_frames(n, N_MAX) for n in (0, 1, 120, 121, 159, 160, 161, 960, 1000, 479999, 480000)] == [2, 2, 2, 3, 3, 3, 3, 8, 8, 3000, 3000]
    assert LR.kept_frames(1600, 1600) == LR.seen_frames(1600, 1600) == 10 and LR.seen_frames(1, 1600) == 2


def test_a_dropped_frame_holds_the_maximum():
    """n = 960: L = 6, and frame 6 -- seen, not kept -- holds the maximum.  A maximum over kept frames alone moves the clamp, and with it
    kept elements; the extractor takes it over all frames."""
    x = LR.dropped_frame_case(1e-6)
    L, A = LR.kept_frames(960, N_MAX), LR.seen_frames(960, N_MAX)
    assert (L, A) == (6, 8)
    lg, out = LR.ref64(x, N_MAX, LR.mel_filters(80))
    assert int(np.argmax(lg.max(axis=0))) == 6
    wrong = LR.finish64(lg, max_frames=L)
    share = float((wrong[:, :L] != out[:, :L]).mean())
    print("maximum over all frames %.3f, over kept frames %.3f; share of kept elements that change %.3f"
          % (lg.max(), lg[:, :L].max(), share))
    assert lg.max() - lg[:, :L].max() > 1.0 and share > 0.0
    got = _extractor()([x], sampling_rate=16000, return_attention_mask=True, padding="max_length", return_tensors="pt")
    feat = got["input_features"][0].numpy().astype(np.float64)
    assert int(got["attention_mask"][0].sum()) == L
    assert np.abs(feat - out).max() <= 1e-4 < np.abs(feat[:, :L] - wrong[:, :L]).max()
