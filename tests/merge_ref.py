"""Torch restatement of the prompt merge (include/x2i_merge.h, x2i_amd/merge.py): both kernels and both plan constructors, on any device.
The kernels copy rows, and multiply token rows by one f32 scale with one rounding -- what torch's bf16 tensor * Python float does -- so
every comparison against these functions is bit for bit and there is no tolerance.  tests/test_merge_ref_cpu.py checks them against the
literal torch forms of the models (scatter over stacked aranges, slice assignment per bound, masked assignment over the flattened batch)."""
import torch

ARRAY_BIT = 30
ROW_MASK = 0x3fffffff


def rank_ref(ids, placeholder):
    """x2i_merge_rank_i32: (src int32 [n], total) -- the exclusive rank of every placeholder row of the flattened ids, -1 elsewhere"""
    hit = ids.reshape(-1) == placeholder
    rank = torch.cumsum(hit.long(), 0) - 1            # inclusive count - 1: the exclusive rank on the rows that hit
    return torch.where(hit, rank, torch.full_like(rank, -1)).to(torch.int32), int(hit.sum())


def src_from_bounds_ref(B, S, image_bound=None, audio_bounds=None):
    """MergePlan.from_bounds' src (a CPU int32 [B * S]): bound by bound, the next rows of the array; audio after vision"""
    src = torch.full((B * S,), -1, dtype=torch.int32)
    for arr, bounds in ((0, image_bound), (1, audio_bounds)):
        n = 0
        for i, sample in enumerate(bounds or []):
            for s, e in sample:
                s, e = int(s), int(e)
                src[i * S + s:i * S + e] = (torch.arange(n, n + e - s) + (arr << ARRAY_BIT)).to(torch.int32)
                n += e - s
    return src


def merge_ref(ids, src, table, scale=1.0, feat0=None, feat1=None, out=None):
    """x2i_embed_merge_bf16 -> (out bf16 [B, S, H], flag): row r is feat_a[k] (a = bit 30 of src[r], k = bits 0..29) when src[r] >= 0, else
    table[ids[r]] * scale as torch multiplies a bf16 tensor by a Python float (scale == 1: the row itself); with table None those rows keep
    what `out` holds.  An id outside the table and a feature row beyond its array give a zero row and flag = 1.  src None: all -1."""
    B, S = ids.shape
    feats = (feat0, feat1)
    H = next(t for t in (table, feat0, feat1) if t is not None).shape[-1]
    dev = ids.device
    out = torch.zeros((B, S, H), dtype=torch.bfloat16, device=dev) if out is None else out.clone()
    flat = out.reshape(B * S, H)
    idf = ids.reshape(-1)
    src = torch.full((B * S,), -1, dtype=torch.int32, device=dev) if src is None else src.reshape(-1)
    flag = 0
    tok = src < 0
    if table is not None:
        ok = tok & (idf >= 0) & (idf < table.shape[0])
        rows = table[idf[ok]]
        flat[ok] = rows if scale == 1.0 else rows * scale
        bad = tok & ~ok
        flat[bad] = 0
        flag |= int(bad.any())
    for a in (0, 1):
        mine = ~tok & ((src >> ARRAY_BIT) & 1 == a)
        k = (src & ROW_MASK).long()
        n = 0 if feats[a] is None else feats[a].shape[0]
        ok = mine & (k < n)
        if feats[a] is not None:
            flat[ok] = feats[a].reshape(-1, H)[k[ok]]
        bad = mine & ~ok
        flat[bad] = 0
        flag |= int(bad.any())
    return flat.reshape(B, S, H), flag
