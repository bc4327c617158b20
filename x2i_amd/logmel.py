"""The Whisper log-mel front end on the HIP path: what `WhisperFeatureExtractor` computes on the host for MiniCPM-o's audio tower -- a
16 kHz waveform to log-mel features [n, n_mels, T] in float32 -- as two launches of libx2i_hip.so (include/ext/x2i_logmel.h,
csrc/logmel.hip).  The tower behind it is x2i_amd/whisper.py.

The definition (frames of 400 samples every 160 with reflect padding, a periodic Hann window, a 201-bin power spectrum, the extractor's
own mel filter bank, log10 with the floor 1e-10, the clamp at the chunk's maximum minus 8, (x + 4) / 4) stands in the header.  Two lengths
belong to a waveform of n samples in a chunk of N = n_samples: L = min(ceil(n / 160), N / 160) frames are KEPT (the extractor's attention
mask), and A = min(N / 160, (n + 199) // 160 + 1) >= L frames can see a sample; the maximum is over all A.

Launch list:
  spectrum   DFT and filter bank on f32-input MFMAs, log10, per-workgroup maxima      x2i_logmel_spectrum_f32
  finish     the maximum, the clamp, zeros from L to T_out, float32 or bf16           x2i_logmel_finish

Host work of a call: the tables are made once, in float64, and rounded to float32 (from_hf); a call on host waveforms copies them into
one pinned buffer and starts one asynchronous transfer (the sample counts ride in the same buffer), a call on device waveforms copies
device to device.  No device-to-host read.  The only wait is for the previous call's transfer out of the same pinned buffer, before it is
overwritten.
"""
import numpy as np
import torch

from . import logmel_binding as lb

N_FFT, HOP, BINS = lb.N_FFT, lb.HOP, lb.BINS


def hann_window():
    """float64 [400]: the periodic Hann window, 0.5 - 0.5 cos(2 pi j / 400)"""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT, dtype=np.float64) / N_FFT)


def dft_table():
    """float64 [400, 448], the layout of include/ext/x2i_logmel.h: row j, column 64 q + c holds w[j] cos(2 pi j k / 400) for c < 32 and
    -w[j] sin(2 pi j k / 400) for c >= 32, k = 32 q + (c mod 32), zero where k >= 201.  The angle is reduced in integers (j k mod 400)."""
    j = np.arange(N_FFT, dtype=np.int64)[:, None]
    k = np.arange(224, dtype=np.int64)[None, :]
    ang = 2.0 * np.pi * ((j * k) % N_FFT).astype(np.float64) / N_FFT
    w = hann_window()[:, None]
    live = (k < BINS).astype(np.float64)
    cos, sin = w * np.cos(ang) * live, -w * np.sin(ang) * live
    tab = np.zeros(lb.DFT_SHAPE, dtype=np.float64)
    for q in range(7):
        tab[:, 64 * q:64 * q + 32] = cos[:, 32 * q:32 * q + 32]
        tab[:, 64 * q + 32:64 * q + 64] = sin[:, 32 * q:32 * q + 32]
    return tab


class LogMelPlan:
    """The buffers of a call on B waveforms of at most ldw samples (LogMel.plan)"""


class LogMel:
    """waveforms -> (features [B, n_mels, T_out] on the device, [L_b]).  mel_filters: [201, n_mels] as WhisperFeatureExtractor holds them;
    n_samples: the chunk length N (a multiple of 160)."""

    def __init__(self, mel_filters, n_samples=480000, device="cuda"):
        f = np.asarray(mel_filters, dtype=np.float64)
        if f.ndim != 2 or f.shape[0] != BINS or not 1 <= f.shape[1] <= lb.MAX_MELS:
            raise ValueError("x2i_amd LogMel: mel_filters must be [201, n_mels] with n_mels in 1..128 (got %s)" % (tuple(f.shape),))
        if n_samples % HOP or n_samples < 2 * HOP or n_samples > 1 << 30:
            raise ValueError("x2i_amd LogMel: n_samples = %r must be a multiple of the hop 160, at least 320" % (n_samples,))
        self.n_mels, self.n_samples, self.device = f.shape[1], int(n_samples), torch.device(device)
        self.T = lb.frames(self.n_samples)
        fb = np.zeros(lb.FBANK_SHAPE, dtype=np.float64)
        fb[:BINS, :self.n_mels] = f
        self.dft = torch.from_numpy(dft_table()).to(torch.float32).to(self.device)
        self.fbank = torch.from_numpy(fb).to(torch.float32).to(self.device)
        self._plan = None

    @classmethod
    def from_hf(cls, feature_extractor, device="cuda"):
        """The front end of a `transformers` WhisperFeatureExtractor: its mel_filters and chunk length.  ValueError, naming the field, for
        what the kernels do not serve."""
        fe = feature_extractor
        if fe.n_fft != N_FFT:
            raise ValueError("x2i_amd LogMel: n_fft = %r; the kernels are built for n_fft = 400" % (fe.n_fft,))
        if fe.hop_length != HOP:
            raise ValueError("x2i_amd LogMel: hop_length = %r; the kernels are built for hop_length = 160" % (fe.hop_length,))
        if fe.n_samples % HOP or fe.n_samples < 2 * HOP:
            raise ValueError("x2i_amd LogMel: n_samples = %r is not a multiple of the hop 160 (at least 320)" % (fe.n_samples,))
        if fe.feature_size > lb.MAX_MELS:
            raise ValueError("x2i_amd LogMel: feature_size = %r; at most 128 mel bins are served" % (fe.feature_size,))
        if getattr(fe, "dither", 0.0) != 0.0:
            raise ValueError("x2i_amd LogMel: dither = %r is not built (0 only)" % (fe.dither,))
        if getattr(fe, "do_normalize", False):
            raise ValueError("x2i_amd LogMel: do_normalize is not built")
        f = np.asarray(fe.mel_filters)
        if f.shape != (BINS, fe.feature_size):
            raise ValueError("x2i_amd LogMel: mel_filters is %s; [201, feature_size = %d] is expected" % (tuple(f.shape), fe.feature_size))
        return cls(f, fe.n_samples, device)

    # ------------------------------------------------------------------ plan
    def plan(self, B, max_samples):
        """The workspaces, the device waveform buffer and the pinned staging buffer of calls on B waveforms of at most max_samples each"""
        B, max_samples = int(B), int(max_samples)
        if B < 1 or not 1 <= max_samples <= self.n_samples:
            raise ValueError("x2i_amd LogMel: a plan needs B >= 1 waveforms of 1..n_samples = %d samples (got B = %d, max_samples = %d)"
                             % (self.n_samples, B, max_samples))
        p = LogMelPlan()
        p.B, p.ldw, p.device = B, (max_samples + 3) // 4 * 4, self.device
        p.head = (4 * B + 15) // 16 * 16                       # the sample counts, then the waveforms, in one buffer: one transfer
        nbytes = p.head + 4 * B * p.ldw
        cuda = self.device.type == "cuda"
        p.stage = torch.empty(nbytes, dtype=torch.uint8, pin_memory=cuda)
        p.dev = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        split = lambda t: (t[:4 * B].view(torch.int32), t[p.head:].view(torch.float32).view(B, p.ldw))   # noqa: E731
        p.stage_n, p.stage_w = split(p.stage)
        p.n, p.wave = split(p.dev)
        lg, part = lb.workspace_floats(B, self.n_samples, self.n_mels)
        p.lg = torch.empty(lg, dtype=torch.float32, device=self.device)
        p.part = torch.empty(part, dtype=torch.float32, device=self.device)
        p.sent = torch.cuda.Event() if cuda else None
        p.busy = False
        return p

    def lengths(self, counts):
        """[L_b] of sample counts: the frames the processor keeps"""
        return [lb.kept_frames(int(n), self.n_samples) for n in counts]

    # ------------------------------------------------------------------ call
    @torch.no_grad()
    def __call__(self, waves, out_dtype=torch.float32, T_out=None, plan=None):
        """waves: a list of 1-D float arrays or tensors, on the host or on the device, each of 1..n_samples samples.  -> (features
        [B, n_mels, T_out] of out_dtype (float32 or bfloat16) on the device, the host list [L_b]); columns L_b .. T_out of sample b are
        zero.  T_out defaults to max L_b."""
        waves = [w if isinstance(w, torch.Tensor) else torch.as_tensor(np.asarray(w)) for w in waves]
        if not waves or any(w.dim() != 1 or not w.is_floating_point() for w in waves):
            raise ValueError("x2i_amd LogMel: waves must be a non-empty list of 1-D float arrays")
        counts = [int(w.shape[0]) for w in waves]
        if min(counts) < 1 or max(counts) > self.n_samples:
            raise ValueError("x2i_amd LogMel: every waveform must hold 1..n_samples = %d samples (got %r); longer audio is cut into chunks "
                             "by the caller" % (self.n_samples, counts))
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("x2i_amd LogMel: out_dtype must be float32 or bfloat16 (got %r)" % (out_dtype,))
        B, Ls = len(waves), self.lengths(counts)
        T_out = max(Ls) if T_out is None else int(T_out)
        if T_out < 1:
            raise ValueError("x2i_amd LogMel: T_out = %d; at least one column is needed" % T_out)
        if plan is None:
            plan = self._plan
            if plan is None or plan.B != B or plan.ldw != (max(counts) + 3) // 4 * 4 or plan.device != self.device:
                plan = self._plan = self.plan(B, max(counts))
        if plan.B != B or plan.ldw < max(counts) or plan.device != self.device:
            raise ValueError("x2i_amd LogMel: the plan is for %d waveforms of at most %d samples on %s; the call holds %d of at most %d on %s"
                             % (plan.B, plan.ldw, plan.device, B, max(counts), self.device))
        if self.device.type != "cuda":
            raise lb.X2IError("x2i_amd: LogMel runs on the GPU only (the module is on %s); there is no CPU fallback" % (self.device,))
        if plan.busy:
            plan.sent.synchronize()                            # the previous transfer out of the staging buffer (long done, as a rule)
        plan.stage_n.copy_(torch.tensor(counts, dtype=torch.int32))
        on_host = all(w.device.type == "cpu" for w in waves)
        if on_host:
            for b, w in enumerate(waves):
                plan.stage_w[b, :counts[b]].copy_(w)
            plan.dev.copy_(plan.stage, non_blocking=True)
        else:
            plan.dev[:plan.head].copy_(plan.stage[:plan.head], non_blocking=True)
            for b, w in enumerate(waves):
                plan.wave[b, :counts[b]].copy_(w, non_blocking=True)
        plan.sent.record()
        plan.busy = True
        out = torch.empty((B, self.n_mels, T_out), dtype=out_dtype, device=self.device)
        lb.spectrum(plan.wave, plan.n, self.dft, self.fbank, plan.lg, plan.part, self.n_samples, self.n_mels)
        lb.finish(plan.lg, plan.part, plan.n, out, self.n_samples, self.n_mels)
        return out, Ls
