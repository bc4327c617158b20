"""The prompt merge on the HIP path (include/x2i_merge.h, x2i_amd/merge_ops.py): which row of layer 0's input comes from where.

A MergePlan has three parts: `src`, one int32 per row of the flattened [B, S] prompt (negative: the token table; otherwise bit 30 picks the
feature array and bits 0..29 the row inside it); up to two feature arrays, vision (array 0) and audio (array 1), with their row counts;
and a device error flag.  Qwen2DecoderStack.forward / prefill take it as `merge=` beside `input_ids` and write the merged rows straight into
entry 0 of their slab with ONE launch: no inputs_embeds tensor, no clone, no scatter, no copy.

Two constructors: from_placeholder ranks the rows that hold a placeholder token on the device (InternVL's `input_embeds[selected] =
vit_embeds.reshape(-1, C)`: no host read), from_bounds builds src on the host from MiniCPM-o's bound lists (get_vllm_embedding's scatter
over stacked aranges, get_omni_embedding's slice assignments): at most one host read for all bounds of a call, none when they are still on
the CPU, and one upload.
"""
import numpy as np
import torch

from . import merge_ops

VISION, AUDIO = 0, 1


def host_ints(*trees):
    """Nested lists / tuples whose leaves are integer tensors on any device (or already numbers) -> the same nesting with every tensor
    replaced by its nested list of Python ints.  All tensors that are not on the CPU cross in ONE concatenated device-to-host copy; with
    none there is no host read at all."""
    pending = []

    def walk(o):
        if isinstance(o, torch.Tensor):
            if o.device.type == "cpu":
                return o.tolist()
            pending.append(o)
            return ("\0slot", len(pending) - 1)
        if isinstance(o, (list, tuple)):
            return [walk(x) for x in o]
        return o

    def fill(o, values):
        if isinstance(o, tuple) and len(o) == 2 and o[0] == "\0slot":
            return values[o[1]]
        if isinstance(o, list):
            return [fill(x, values) for x in o]
        return o

    walked = [walk(t) for t in trees]
    if not pending:
        return walked
    host = torch.cat([t.reshape(-1).long() for t in pending]).cpu()      # the one host read
    values, at = [], 0
    for t in pending:
        values.append(host[at:at + t.numel()].reshape(t.shape).tolist())
        at += t.numel()
    return [fill(w, values) for w in walked]


class MergePlan:
    """src int32 [B * S] on the device; feats: [vision, audio], each None or a bf16 [rows, H] tensor with contiguous rows; err int32 [1].
    expect: per array the number of rows src asks for, a host int (from_bounds), or None when only the device knows it (`total`, from_placeholder).
    check=True (the default) reads the device ONCE after the merge launch and raises ValueError on the error flag (an id outside the
    table, a feature row beyond its array) and on a placeholder total that differs from the feature rows; a bound total that differs is
    refused before the launch, with or without check.  check=False skips the read."""

    def __init__(self, B, S, src, expect, total=None, check=True):
        self.B, self.S, self.src, self.expect, self.total, self.check = B, S, src, list(expect), total, check
        self.feats = [None, None]
        self.err = torch.zeros((1,), device=src.device, dtype=torch.int32)

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_placeholder(cls, input_ids, token_id, check=True):
        """Every row of input_ids [B, S] (int64, on the GPU) that equals token_id takes the next row of the vision array, in the row order of the
        flattened batch: the rank kernel, no host read."""
        if input_ids.dim() != 2:
            raise ValueError("MergePlan.from_placeholder: input_ids must be [B, S] (got %s)" % (tuple(input_ids.shape),))
        ids = input_ids.contiguous()
        B, S = ids.shape
        dev = ids.device
        src = torch.empty((B * S,), device=dev, dtype=torch.int32)
        total = torch.empty((1,), device=dev, dtype=torch.int32)
        ws = torch.empty((merge_ops.rank_workspace_ints(B * S),), device=dev, dtype=torch.int32)
        merge_ops.rank(ids, int(token_id), src, total, ws)
        return cls(B, S, src, [None, 0], total=total, check=check)

    @staticmethod
    def src_from_bounds(B, S, image_bound=None, audio_bounds=None, vision_rows=None, audio_rows=None):
        """(src as a numpy int32 [B * S], [vision rows, audio rows]) of host bound lists: sample by sample and bound by bound, rows [start, end)
        of the sample take the next end - start rows of their array (vision rows are counted over the whole batch, as the model's
        vision_embedding is one array over all images; so are the audio rows).  Audio bounds are applied after the image bounds, as
        get_omni_embedding runs after get_vllm_embedding.  vision_rows / audio_rows: per sample the feature rows that sample owns; its
        bounds must ask for exactly that many (ValueError), which is what keeps a sample's rows its own."""
        src = np.full((B * S,), -1, dtype=np.int32)
        counts = [0, 0]
        for arr, bounds, own, name in ((VISION, image_bound, vision_rows, "vision"), (AUDIO, audio_bounds, audio_rows, "audio")):
            if bounds is None:
                bounds = []
            if own is not None:
                asked = [sum(e - s for s, e in sample) for sample in bounds] + [0] * (len(own) - len(bounds))
                if asked != [int(n) for n in own] + [0] * (len(asked) - len(own)):
                    raise ValueError("MergePlan.from_bounds: the bounds ask for %r %s rows per sample and the features have %r" % (asked, name, list(own)))
            if len(bounds) > B:
                raise ValueError("MergePlan.from_bounds: %d bound lists for a batch of %d" % (len(bounds), B))
            for i, sample in enumerate(bounds):
                for s, e in sample:
                    if not 0 <= s <= e <= S:
                        raise ValueError("MergePlan.from_bounds: the bound [%d, %d) of sample %d does not lie in a prompt of %d rows" % (s, e, i, S))
                    src[i * S + s:i * S + e] = np.arange(counts[arr], counts[arr] + e - s, dtype=np.int32) | (arr << merge_ops.SRC_ARRAY_BIT)
                    counts[arr] += e - s
        return src, counts

    @classmethod
    def from_bounds(cls, B, S, image_bound=None, audio_bounds=None, device="cuda", check=True, vision_rows=None, audio_rows=None):
        """image_bound / audio_bounds: per sample the [start, end) row ranges that the vision / audio rows fill, in order (MiniCPM-o's
        processor outputs: tensors [n, 2] on any device, or lists of pairs).  At most one host read for all of them (host_ints), one upload."""
        image_bound, audio_bounds = host_ints(image_bound, audio_bounds)
        src, counts = cls.src_from_bounds(B, S, image_bound, audio_bounds, vision_rows, audio_rows)
        return cls(B, S, torch.from_numpy(src).to(device), counts, check=check)

    # ------------------------------------------------------------------ features
    def set_features(self, vision=None, audio=None):
        """The feature arrays: bf16 tensors whose last dimension is H, flattened to [rows, H] views (no copy when the rows are contiguous)"""
        for arr, t in ((VISION, vision), (AUDIO, audio)):
            if t is not None:
                t = t.reshape(-1, t.shape[-1])
                if t.stride(1) != 1:
                    t = t.contiguous()
            self.feats[arr] = t
        return self

    def _refuse_host_totals(self):
        for arr, name in ((VISION, "vision"), (AUDIO, "audio")):
            have = 0 if self.feats[arr] is None else self.feats[arr].shape[0]
            if self.expect[arr] is not None and self.expect[arr] != have:
                raise ValueError("MergePlan: the bounds ask for %d %s rows and the features have %d" % (self.expect[arr], name, have))

    # ------------------------------------------------------------------ the launch
    def launch(self, out, input_ids=None, table=None, scale=1.0):
        """out [B, S, H] (a view such as slab[:, 0]) <- the merged rows: ONE launch.  table None: overwrite mode (only the feature rows are
        written).  Then, with check, the one host read."""
        if tuple(out.shape[:2]) != (self.B, self.S):
            raise ValueError("MergePlan: planned for [B, S] = [%d, %d], asked to fill %s" % (self.B, self.S, tuple(out.shape)))
        self._refuse_host_totals()
        self.err.zero_()
        ids = None if input_ids is None else input_ids.contiguous()
        merge_ops.embed_merge(out, self.err, ids=ids, src=self.src, table=table, scale=scale, feat0=self.feats[VISION], feat1=self.feats[AUDIO])
        if self.check:
            self.verify()
        return out

    def verify(self):
        """One host read: the error flag, and the placeholder total where only the device knows it.  Raises ValueError."""
        if self.total is not None:
            err, total = torch.cat((self.err, self.total)).tolist()
            have = 0 if self.feats[VISION] is None else self.feats[VISION].shape[0]
            if total != have:
                raise ValueError("MergePlan: the prompt holds %d placeholder rows and the features have %d" % (total, have))
        else:
            err = int(self.err.item())
        if err:
            raise ValueError("MergePlan: the merge met a token id outside the table or a feature row beyond its array (those rows are zeros)")
