"""The log-mel front end's kernels (csrc/logmel.hip) on the GPU against the float64 reference of tests/logmel_ref.py.

The float32 bound is per input: the kernel's worst absolute error over a sample's kept frames is at most 4 times the worst error of the
float32 restatement (torch CPU matmuls, another summation order) on the same elements, plus 1e-6.  The bf16 output is the rounding of the
same launch's float32 output, bit for bit; against the rounded float64 reference two roundings of values that differ by d land at most
one step apart where a step is at least d, so: at most one bf16 ulp off wherever the ulp is at least that input's float32 bound E, at
most E plus one ulp where it is smaller (values next to zero), and different at all on at most 1e-3 of the kept elements.

Measured (profiles/logmel_gputest.log): see DESIGN.md section 4, "Whisper log-mel front end".
"""
import functools

import numpy as np
import pytest
import torch

from tests import logmel_ref as LR
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

G = 256                       # guard elements on either side of every buffer
CANARY = 777.0
CASES = [(480000, 80), (480000, 128), (1600, 80)]


@functools.lru_cache(maxsize=None)
def _batch(N_max):
    return LR.edge_batch(N_max)


@functools.lru_cache(maxsize=None)
def _power(N_max, b):
    return LR.power64(_batch(N_max)[b], N_max)


@functools.lru_cache(maxsize=None)
def _reference(N_max, n_mels):
    """per sample: (float64 out [n_mels, L], the float32 restatement's worst error on those elements)"""
    f = LR.mel_filters(n_mels)
    res = []
    for b, x in enumerate(_batch(N_max)):
        L = LR.kept_frames(len(x), N_max)
        out = LR.ref64(x, N_max, f, power=_power(N_max, b))[1][:, :L]
        res.append((out, float(np.abs(LR.restate32(x, N_max, f)[:, :L].astype(np.float64) - out).max())))
    return res


def _guarded(numel, dtype=torch.float32):
    t = torch.full((numel + 2 * G,), CANARY, dtype=dtype, device="cuda")
    return t, t[G:G + numel]


def _intact(t):
    return bool((t[:G] == CANARY).all()) and bool((t[-G:] == CANARY).all())


class Rig:
    """Tables, guarded buffers and the two launches for one batch of waveforms"""

    def __init__(self, waves, N_max, n_mels, T_out, dtype=torch.float32, pad=3):
        from x2i_amd import logmel_binding as lb
        from x2i_amd.logmel import LogMel
        self.lb, self.N_max, self.n_mels, self.T_out, self.B = lb, N_max, n_mels, T_out, len(waves)
        self.lm = LogMel(LR.mel_filters(n_mels), N_max, "cuda")
        self.counts = [len(w) for w in waves]
        B, ldw = self.B, max(self.counts)
        self.wave_all, wave = _guarded(B * ldw)
        self.wave = wave.view(B, ldw)
        for b, w in enumerate(waves):
            self.wave[b, :len(w)] = torch.from_numpy(w).cuda()
        self.n = torch.tensor(self.counts, dtype=torch.int32, device="cuda")
        lgf, pf = lb.workspace_floats(B, N_max, n_mels)
        self.lg_all, self.lg = _guarded(lgf)
        self.part_all, self.part = _guarded(pf)
        self.ld = T_out + pad
        self.out_all, out = _guarded(B * n_mels * self.ld, dtype)
        self.out_rows = out.view(B, n_mels, self.ld)
        self.out = self.out_rows[:, :, :T_out]

    def spectrum(self):
        self.lb.spectrum(self.wave, self.n, self.lm.dft, self.lm.fbank, self.lg, self.part, self.N_max, self.n_mels)
        return self

    def finish(self):
        self.lb.finish(self.lg, self.part, self.n, self.out, self.N_max, self.n_mels)
        return self

    def intact(self):
        return (_intact(self.wave_all) and _intact(self.lg_all) and _intact(self.part_all) and _intact(self.out_all)
                and bool((self.out_rows[:, :, self.T_out:] == CANARY).all()))


@pytest.mark.parametrize("N_max,n_mels", CASES)
def test_batch_against_the_float64_reference(N_max, n_mels):
    waves, ref = _batch(N_max), _reference(N_max, n_mels)
    T = N_max // 160
    Ls = [LR.kept_frames(len(w), N_max) for w in waves]
    T_out = max(Ls) + 5                                   # beyond T: columns of zeros
    rig = Rig(waves, N_max, n_mels, T_out).spectrum().finish()
    torch.cuda.synchronize()
    assert rig.intact()
    got = rig.out.cpu().numpy()
    # the spectrum launch wrote the frames of the workgroups that can see a sample, nothing else
    lg, part = rig.lg.view(rig.B, n_mels, T).cpu(), rig.part.view(rig.B, -1).cpu()
    for b, w in enumerate(waves):
        nb = -(-LR.seen_frames(len(w), N_max) // 32)
        assert bool((lg[b, :, 32 * nb:] == CANARY).all()) and bool((part[b, nb:] == CANARY).all())
        assert bool((lg[b, :, :min(32 * nb, T)] != CANARY).all()) and bool((part[b, :nb] >= -10.0).all()) and bool((lg[b, :, :min(32 * nb, T)] >= -10.0).all())
    # float32 against float64, input by input
    bounds = []
    for b, (want, rest) in enumerate(ref):
        L = Ls[b]
        err = float(np.abs(got[b, :, :L].astype(np.float64) - want).max())
        bounds.append(4.0 * rest + 1e-6)
        print("N_max=%d n_mels=%d n=%d L=%d: kernel %.3g, float32 restatement %.3g, bound %.3g" % (N_max, n_mels, len(waves[b]), L, err, rest, bounds[b]))
        assert not got[b, :, L:].any()                    # the processor's pad value
    for b, (want, rest) in enumerate(ref):
        assert float(np.abs(got[b, :, :Ls[b]].astype(np.float64) - want).max()) <= bounds[b], (b, len(waves[b]))
    assert (got[-1, :, :Ls[-1]] == -1.5).all()            # the all-zero sample, exactly
    # bf16: the rounding of the same launch's float32 output
    rig16 = Rig(waves, N_max, n_mels, T_out, torch.bfloat16)
    rig16.lg.copy_(rig.lg)
    rig16.part.copy_(rig.part)
    rig16.finish()
    torch.cuda.synchronize()
    assert rig16.intact() and torch.equal(rig16.out, rig.out.to(torch.bfloat16))
    got16 = rig16.out.float().cpu().numpy().astype(np.float64)
    differ = total = 0
    for b, (want, _) in enumerate(ref):
        L = Ls[b]
        want16 = torch.from_numpy(want).to(torch.bfloat16).double().numpy()
        d = np.abs(got16[b, :, :L] - want16)
        ulp = LR.ulp_bf16(np.maximum(np.abs(want16), np.abs(got16[b, :, :L])))
        assert (d <= np.where(ulp >= bounds[b], ulp, bounds[b] + ulp)).all(), (b, float((d / ulp).max()))
        differ, total = differ + int((d != 0).sum()), total + d.size
    print("N_max=%d n_mels=%d bf16: %d of %d kept elements differ from the rounded float64 reference (%.3g)" % (N_max, n_mels, differ, total, differ / total))
    assert differ <= 1e-3 * total
    # a relaunch, and another T_out, change no bit
    again = Rig(waves, N_max, n_mels, T_out).spectrum().finish()
    short = Rig(waves, N_max, n_mels, max(Ls))
    short.lg.copy_(rig.lg)
    short.part.copy_(rig.part)
    short.finish()
    torch.cuda.synchronize()
    assert torch.equal(again.out, rig.out) and torch.equal(again.lg, rig.lg) and torch.equal(again.part, rig.part)
    assert short.intact() and torch.equal(short.out, rig.out[:, :, :max(Ls)])


@pytest.mark.parametrize("N_max,n_mels", [(480000, 80), (1600, 80)])
def test_a_sample_alone_is_bit_equal_to_its_rows_in_the_batch(N_max, n_mels):
    waves = _batch(N_max)
    Ls = [LR.kept_frames(len(w), N_max) for w in waves]
    rig = Rig(waves, N_max, n_mels, max(Ls)).spectrum().finish()
    for b, w in enumerate(waves):
        one = Rig([w], N_max, n_mels, Ls[b]).spectrum().finish()          # its own ldw, its own T_out
        torch.cuda.synchronize()
        assert one.intact() and torch.equal(one.out[0], rig.out[b, :, :Ls[b]]), (b, len(w))


def test_bad_arguments_are_refused_before_any_launch():
    from x2i_amd._lib import X2IError
    waves = _batch(1600)[:3]
    rig = Rig(waves, 1600, 80, 4)
    lb = rig.lb
    calls = [
        (lambda: lb.spectrum(rig.wave, rig.n, rig.lm.dft, rig.lm.fbank, rig.lg, rig.part, 1601, 80), r"code -2.*N_max=1601"),
        (lambda: lb.spectrum(rig.wave, rig.n, rig.lm.dft, rig.lm.fbank, rig.lg, rig.part, 1600, 129), r"code -2.*n_mels=129"),
        (lambda: lb.spectrum(rig.wave, rig.n, rig.lm.dft, rig.lm.fbank, rig.lg[:-1], rig.part, 1600, 80), r"code -1.*lg_floats"),
        (lambda: lb.spectrum(rig.wave, rig.n, rig.lm.dft, rig.lm.fbank, rig.lg, rig.part[:-1], 1600, 80), r"code -1.*part_floats"),
        (lambda: lb.spectrum(rig.wave, rig.n, rig.lm.dft[:, :-1], rig.lm.fbank, rig.lg, rig.part, 1600, 80), r"dft must be"),
        (lambda: lb.spectrum(rig.wave, rig.n[:2], rig.lm.dft, rig.lm.fbank, rig.lg, rig.part, 1600, 80), r"sample counts"),
        (lambda: lb.spectrum(rig.wave.double(), rig.n, rig.lm.dft, rig.lm.fbank, rig.lg, rig.part, 1600, 80), r"wave must be"),
        (lambda: lb.spectrum(rig.wave.cpu(), rig.n, rig.lm.dft, rig.lm.fbank, rig.lg, rig.part, 1600, 80), r"must live on the GPU"),
        (lambda: lb.finish(rig.lg, rig.part, rig.n, rig.out, 1500, 80), r"code -2.*N_max=1500"),
        (lambda: lb.finish(rig.lg, rig.part, rig.n, rig.out, 1600, 80, T_out=0), r"code -2.*T_out=0"),
        (lambda: lb.finish(rig.lg, rig.part, rig.n, rig.out, 1600, 80, T_out=5), r"out holds"),
        (lambda: lb.finish(rig.lg[:-1], rig.part, rig.n, rig.out, 1600, 80), r"code -1.*lg_floats"),
        (lambda: lb.finish(rig.lg, rig.part, rig.n, rig.out.half(), 1600, 80), r"float32 or bfloat16"),
        (lambda: lb.finish(rig.lg, rig.part, rig.n, rig.out[:, :79], 1600, 80), r"n_mels = 80"),
    ]
    for call, msg in calls:
        with pytest.raises(X2IError, match=msg):
            call()
    torch.cuda.synchronize()
    assert rig.intact()
    for t in (rig.lg, rig.part, rig.out):
        assert bool((t == CANARY).all())                   # nothing ran


def test_logmel_on_host_and_on_device_inputs_agree_bit_for_bit():
    from x2i_amd.logmel import LogMel
    from transformers import WhisperFeatureExtractor
    waves = _batch(480000)
    lm = LogMel.from_hf(WhisperFeatureExtractor(), "cuda")
    host, Ls = lm(waves)
    dev, Ls2 = lm([torch.from_numpy(w).cuda() for w in waves])
    mixed, _ = lm([w if b % 2 else torch.from_numpy(w).double().cuda() for b, w in enumerate(waves)])
    rig = Rig(waves, 480000, 80, max(Ls)).spectrum().finish()
    assert Ls == Ls2 == [LR.kept_frames(len(w), 480000) for w in waves] and host.shape == (len(waves), 80, 3000) and host.dtype == torch.float32
    assert torch.equal(host, dev) and torch.equal(host, mixed) and torch.equal(host, rig.out)
    # lists of floats and float64 arrays are waveforms too; another batch size makes another plan; T_out pads with zeros
    few, L3 = lm([waves[5].astype(np.float64), waves[0].tolist()], out_dtype=torch.bfloat16, T_out=9)
    assert L3 == [7, 1] and few.shape == (2, 80, 9) and few.dtype == torch.bfloat16
    assert torch.equal(few[0, :, :7], host[5, :, :7].to(torch.bfloat16)) and torch.equal(few[1, :, :1], host[0, :, :1].to(torch.bfloat16))
    assert not bool(few[0, :, 7:].any()) and not bool(few[1, :, 1:].any())
    host2, _ = lm(waves)                                   # the staging buffer is reused
    assert torch.equal(host2, host)


def test_hip_logmel_feeds_the_audio_tower_on_device_tensors():
    from transformers import WhisperFeatureExtractor
    from tests.test_logmel_handoff_cpu import StubProcessor
    from x2i_amd import handoff
    from x2i_amd.whisper import WhisperAudioTower
    tower = WhisperAudioTower(d_model=128, encoder_attention_heads=2, encoder_ffn_dim=256, encoder_layers=2, max_source_positions=150,
                              embed_dim=96, pool_step=2, device="cuda").init_random_(seed=5)
    sig = LR.six_signals()
    waves = [sig["chirp"][:40000], sig["clip"], LR.dropped_frame_case(1e-3)]
    proc = StubProcessor(WhisperFeatureExtractor())
    want_feats, want_lens = proc.audio_features(waves)    # the host path
    with handoff.HipLogMel(proc) as hm:
        feats, lens = proc.audio_features(waves)
        assert hm.calls == 1
    assert feats.is_cuda and feats.dtype == torch.float32 and feats.shape == want_feats.shape == (3, 80, 250) and lens.device.type == "cpu"
    assert lens.tolist() == want_lens.tolist() == [250, 7, 6]
    assert float((feats.cpu() - want_feats).abs().max()) <= 2e-4      # each side within 1e-4 of the float64 reference
    out, counts = tower(feats, feature_lens=lens.tolist())
    ref, counts2 = tower(want_feats.cuda(), feature_lens=want_lens.tolist())
    torch.cuda.synchronize()
    assert counts == counts2 and out.shape == ref.shape and bool(torch.isfinite(out.float()).all())
    # the tower rounds its input to bf16: features 2e-4 apart differ in a few last bits of that rounding
    for b, n in enumerate(counts):
        assert rel_l2(out[b, :n], ref[b, :n]) < 1e-2
