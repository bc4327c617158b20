"""x2i_sample_select_f32 (include/ext/sample/x2i_sample.h, csrc/qwen_sample.hip) on the GPU against the float64 reference of
tests/sample_ref.py: synthetic f32 scores and a hand-filled head workspace, no lm_head and no weight.  The cases, their inputs, the
allowance eps with its derivation and the coverage conditions every case asserts before it launches are in tests/sample_ref.py.
The largest share of eps a draw used goes to profiles/sample_gputest.log.

Measured on the MI355X: see DESIGN.md section 4, "Sampled token selection".
"""
import os

import numpy as np
import pytest
import torch

from tests import sample_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_STEP = -2 ** 31


@pytest.fixture(scope="module")
def sb():
    from x2i_amd import sample_binding
    sample_binding.load()
    return sample_binding


@pytest.fixture(scope="module")
def worst():
    w = dict(share=0.0, where="none: every token's exact interval held its u", z=0.0, z_where="")
    yield w
    try:
        with open(os.path.join(ROOT, "profiles", "sample_gputest.log"), "w") as f:
            f.write("tests/test_sample_gpu.py: largest share of eps a draw used: %.4f (%s)\n" % (w["share"], w["where"]))
            f.write("tests/test_sample_gpu.py: largest share of eps * Z by which a launch's Z differed from the float64 Z: %.4f (%s)\n"
                    % (w["z"], w["z_where"]))
    except OSError:
        pass


def workspace(p, col):
    """The head launch's workspace for the f32 scores p [B, V], filled by hand: the counter's snapshot, then per (sample, 16 rows) the largest
    score and its lowest index"""
    B, V = p.shape
    nwg = (V + 15) // 16
    pad = np.full((B, nwg * 16), -np.inf, np.float32)
    pad[:, :V] = p
    pad = pad.reshape(B, nwg, 16)
    part = np.empty((B, nwg, 2), np.float32)
    part[..., 0] = pad.max(-1)
    part[..., 1] = (pad.argmax(-1) + 16 * np.arange(nwg)[None]).astype(np.int32).view(np.float32)
    ws = np.zeros(4 + 2 * B * nwg, np.float32)
    ws[:1] = np.array([col], np.int32).view(np.float32)
    ws[4:] = part.reshape(-1)
    return torch.from_numpy(ws).to(DEV)


class State:
    def __init__(self, B, V, ncols=16, col=3, eos=(), seen=True):
        self.step = torch.tensor([col if col != NO_STEP else 0], device=DEV, dtype=torch.int32)
        self.token = torch.full((B,), -7, device=DEV, dtype=torch.int64)
        self.seq = torch.full((B, ncols), -1, device=DEV, dtype=torch.int64)
        self.lengths = torch.zeros((B,), device=DEV, dtype=torch.int64)
        self.done = torch.zeros((B,), device=DEV, dtype=torch.uint8)
        self.eos = torch.tensor(list(eos), device=DEV, dtype=torch.int64) if eos else None
        self.seen = torch.zeros((B, V), device=DEV, dtype=torch.uint8) if seen else None
        self.diag = torch.full((B, 4), -1.0, device=DEV, dtype=torch.float32)


def launch(sb, logits, ws, case, st, u=None, rng=None, pad=0):
    sb.select(logits, ws, st.step, st.token, st.seq, st.lengths, st.done, pad, temperature=case["temperature"], top_k=case["top_k"],
              top_p=case["top_p"], rng=rng, u=u, diag=st.diag, eos=st.eos, seen=st.seen)
    return st.token.cpu().numpy(), st.diag.cpu().numpy()


@pytest.mark.parametrize("case", R.cases(), ids=lambda c: c["id"])
def test_draws_pass_the_verdict(sb, worst, case):
    assert R.coverage(case) == []                                  # before any launch: the margin at the top-p cut, one token per draw
    B, V = case["B"], case["V"]
    p = R.rows(case)
    buf = torch.full((B, V + 3), 1e30, device=DEV, dtype=torch.float32)        # (a padded row stride: rows that are not 16-byte aligned)
    logits = buf[:, :V]
    logits.copy_(torch.from_numpy(p))
    refs = [R.reference(case, b) for b in range(B)]
    draws = [R.us(case, b) for b in range(B)]
    ws = workspace(p, 3)
    first = None
    for i in range(len(draws[0])):
        key = draws[0][i][1]
        st = State(B, V)
        if key is None:
            tok, diag = launch(sb, logits, ws, case, st, u=torch.tensor([float(draws[b][i][0]) for b in range(B)], device=DEV))
        else:
            seed, offset, col = key
            tok, diag = launch(sb, logits, workspace(p, col), case, st, rng=sb.rng_state(seed, offset, DEV))
        for b in range(B):
            u = draws[b][i][0]
            assert diag[b, 3].view(np.uint32) == np.float32(u).view(np.uint32), (b, i, diag[b, 3], u)      # the numpy Philox, bit for bit
            bad = R.verdict(refs[b], tok[b], u, diag[b, 0], diag[b, 2])
            assert not bad, "%s sample %d draw %d: %s" % (case["id"], b, i, bad)
            assert diag[b, 1] == refs[b].s_min
            sh = R.share(refs[b], int(tok[b]), u)
            if sh > worst["share"]:
                worst.update(share=sh, where="%s sample %d u=%.9g" % (case["id"], b, u))
            zs = abs(float(diag[b, 2]) - refs[b].Z) / (R.eps(refs[b].count) * refs[b].Z)
            if zs > worst["z"]:
                worst.update(z=zs, z_where="%s sample %d" % (case["id"], b))
        if i == 2:
            first = tok.copy()
            for _ in range(2):                                       # three launches agree
                again, d2 = launch(sb, logits, ws, case, State(B, V), u=torch.tensor([float(draws[b][i][0]) for b in range(B)], device=DEV))
                assert np.array_equal(again, first) and np.array_equal(d2, diag)
            if B > 1:                                                # a sample alone at B = 1, in row 0 of another buffer
                for b in (B - 1, B // 2):
                    alone = torch.from_numpy(p[b:b + 1]).to(DEV)
                    t1, d1 = launch(sb, alone, workspace(p[b:b + 1], 3), dict(case, B=1), State(1, V),
                                    u=torch.tensor([float(draws[b][i][0])], device=DEV))
                    assert t1[0] == first[b] and np.array_equal(d1[0], diag[b])


def test_top_k_1_is_the_argmax_of_the_greedy_select(sb):
    from x2i_amd import qwen_head_ops as ho
    for B, V in ((3, 1000), (8, 4099), (1, 151936)):
        p = np.stack([R.scores("normal", V, 77 + b) for b in range(B)])
        p[0, V // 2] = p[0, V - 1] = p[0].max() + 1                 # equal maxima: the lowest index, with u = 0
        ws, logits = workspace(p, 2), torch.from_numpy(p).to(DEV)
        g, s = State(B, V), State(B, V)
        ho.select(ws, g.step, g.token, g.seq, g.lengths, g.done, 0, V, seen=g.seen)
        tok, diag = launch(sb, logits, ws, dict(temperature=0.7, top_k=1, top_p=1.0), s, u=torch.zeros(B, device=DEV))
        assert np.array_equal(tok, g.token.cpu().numpy()) and np.array_equal(tok, p.argmax(-1))
        for a, b in ((g.seq, s.seq), (g.lengths, s.lengths), (g.done, s.done), (g.seen, s.seen), (g.step, s.step)):
            assert torch.equal(a, b)
        assert diag[0, 0] == 2 and (diag[1:, 0] == 1).all()


def test_bookkeeping_follows_the_greedy_selects_rules(sb):
    B, V, pad = 3, 17, 5
    p = np.stack([R.scores("normal", V, 5 + b) for b in range(B)])
    want = p.argmax(-1)
    logits, case = torch.from_numpy(p).to(DEV), dict(temperature=1.0, top_k=1, top_p=1.0)
    u = torch.full((B,), 0.5, device=DEV)
    # sample 1 is done already; sample 2's token is an end token
    st = State(B, V, ncols=8, col=3, eos=(int(want[2]), 16))
    st.done[1] = 1
    tok, _ = launch(sb, logits, workspace(p, 3), case, st, u=u, pad=pad)
    assert tok.tolist() == [want[0], pad, want[2]]
    assert st.seq[:, 3].tolist() == tok.tolist() and int((st.seq != -1).sum()) == B
    assert st.lengths.tolist() == [1, 0, 1] and st.done.tolist() == [0, 1, 1] and st.step.item() == 4
    seen = torch.zeros((B, V), dtype=torch.uint8)
    seen[torch.arange(B), torch.from_numpy(tok)] = 1
    assert torch.equal(st.seen.cpu(), seen)
    # a column outside [0, ncols): nothing of sequences is written, everything else is, and the counter still advances
    for col in (8, -1, 2 ** 31 - 2):
        st = State(B, V, ncols=8, col=col)
        tok, _ = launch(sb, logits, workspace(p, col), case, st, u=u, pad=pad)
        assert tok.tolist() == want.tolist() and bool((st.seq == -1).all()) and st.lengths.tolist() == [1, 1, 1] and st.step.item() == col + 1
    # no counter (the logits call had step = NULL) and the largest int: no column and no advance
    for col in (NO_STEP, 2 ** 31 - 1):
        st = State(B, V, ncols=8, col=col, seen=False)
        st.step.fill_(123)
        tok, _ = launch(sb, logits, workspace(p, col), case, st, u=u, pad=pad)
        assert tok.tolist() == want.tolist() and bool((st.seq == -1).all()) and st.step.item() == 123


def test_every_token_is_in_the_vocabulary_whatever_the_buffers_hold(sb):
    B, V = 2, 1000
    p = np.stack([R.scores("normal", V, 9 + b) for b in range(B)])
    p[0, ::3] = np.nan
    p[1, 5] = np.inf
    ws = workspace(np.nan_to_num(p, nan=0.0, posinf=0.0), 1)
    ws[4:] = torch.from_numpy(np.random.default_rng(1).standard_normal(ws.numel() - 4).astype(np.float32) * 1e30)      # partials of nonsense
    for k, pp in ((0, 1.0), (50, 0.8), (1, 1e-6)):
        st = State(B, V)
        tok, _ = launch(sb, torch.from_numpy(p).to(DEV), ws, dict(temperature=0.7, top_k=k, top_p=pp), st, u=torch.tensor([0.3, 0.99], device=DEV))
        assert ((0 <= tok) & (tok < V)).all()
