"""The checker of tests/proj_ref.py is itself tested, without a GPU:

  * the reference is right: conv5x5_sums equals float64 F.conv2d on the same operands, pack_expect equals a loop over the documented index
    formula;
  * f32 stand-ins, written in plain torch, that follow each kernel form's summation order (the VALU form's dot2 chains; the MFMA forms'
    per-kernel-row accumulators and five-term epilogue; the two means' chains) stay inside the derived allowance on every operand kind at
    C in {1, 8, 37, 64} -- asserted, the share printed;
  * every planted fault passes the old whole-tensor check (proj_ref.OLD_*; computed here, not assumed) and is rejected by the new checker
    at the expected form, sample, row, column and block."""
import pytest
import torch
import torch.nn.functional as F

from tests import proj_ref as R

BF = torch.bfloat16


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def wb_of(w):
    """the taps as the kernels use them: bf16 (RNE), as f32 [1, C, 5, 5]"""
    return w.to(BF).float().view(1, -1, 5, 5)


# ---------------------------------------------------------------------------------------------------------------- the reference is right
@pytest.mark.parametrize("kind", R.CONV_KINDS)
@pytest.mark.parametrize("B,C,S,H", [(1, 1, 1, 8), (2, 5, 7, 24), (1, 37, 20, 40)])
def test_reference_equals_torch_conv(kind, B, C, S, H):
    x, w, bias = R.conv_operands(kind, B, C, S, H, gen(1))
    ref = F.conv2d(x.double(), wb_of(w).double(), bias.double(), padding=2)[:, 0]
    for z in range(B):
        for r0, r1 in ((0, S), (S // 2, S), (0, max(1, S // 3))):
            lin, mag = R.conv5x5_sums(x[z], w, r0, r1)
            assert float((lin + bias.double() - ref[z, r0:r1]).abs().max()) <= 1e-13 * float(mag.max() + 1.0), (z, r0, r1)
            mref = F.conv2d(x[z:z + 1].double().abs(), wb_of(w).double().abs(), padding=2)[0, 0, r0:r1]
            assert float((mag - mref).abs().max()) <= 1e-13 * float(mref.max())
    want, bound, d = R.conv5x5_expect(x[0], w, bias, "valu1")
    assert bool((bound > d).all()) and bool((d > 0).all())


def test_integer_operands_are_exact():
    x = torch.randint(-4, 5, (1, 6, 9, 16), generator=gen(2)).to(BF)
    w = torch.randint(-3, 4, (6, 25), generator=gen(3)).float()
    lin, _ = R.conv5x5_sums(x[0], w, 0, 9)
    assert torch.equal(lin, F.conv2d(x.double(), w.double().view(1, 6, 5, 5), padding=2)[0, 0])


def test_pack_expect_is_the_documented_table():
    w = torch.randn((3, 25), generator=gen(4))
    t = R.pack_expect(w)
    wb = w.to(BF).view(3, 5, 5)
    for c in range(3):
        for ds in range(5):
            for lane in range(64):
                n, g = lane % 16, lane // 16
                for j in range(8):
                    dh = 8 * g + j - n - 6
                    want = wb[c, ds, dh] if 0 <= dh <= 4 else torch.zeros((), dtype=BF)
                    assert t[c, ds, lane, j].view(torch.int16) == want.view(torch.int16)
    assert int((t != 0).sum()) <= 3 * 5 * 16 * 5         # five taps per Toeplitz row


def test_dispatch_mirrors():
    """the shapes the GPU test relies on: one tile below the VALU threshold, the three two-stream shapes, the self-chosen two-row-block form"""
    assert R.valu_form(2, 1360, 1032) == "valu1" and R.valu_form(2, 1361, 1032) == "valu2"
    assert R.valu_form(2, 1384, 1032) == "valu2" and R.valu_form(2, 1376, 1032) == "valu2" and R.valu_form(2, 40, 896) == "valu1"
    assert R.mfma_tiles2(1, 1248, 1032) == 260 and R.mfma_form(0, 1, 1248, 1032) == "mfma_rb2"
    assert R.mfma_form(0, 3, 40, 512) == "mfma_pipe" and R.mfma_form(3, 3, 40, 512) == "mfma_rb2" and R.mfma_form(1, 3, 40, 512) == "mfma_pair"
    assert R.conv5x5_depth("valu1", 37) == 3 * 5 * 40 * 2 + 1 and R.conv5x5_depth("mfma_rb2", 37) == 5 * 37 + 5


# ---------------------------------------------------------------------------------------------------------------- f32 stand-ins
def valu_standin(x, w, bias):
    """csrc/projector.hip in f32 for one sample x [C, S, H]: per output one accumulator; input rows in order (kernel row 0 first), the layers
    in order, three dot2 per layer -- an even column pairs the taps (w0 w1)(w2 w3)(w4 0), an odd one (0 w0)(w1 w2)(w3 w4) -- each dot2 as two
    rounded adds of exact products; then the bias"""
    C, S, H = x.shape
    wb = w.to(BF).float().view(C, 5, 5)
    xp = F.pad(x.float(), (3, 3, 2, 2))
    even = (torch.arange(H) % 2 == 0)[None, :]
    acc = torch.zeros((S, H))
    zero = torch.zeros((S, H))
    for di in range(5):
        for c in range(C):
            X = lambda k: xp[c, di:di + S, 3 + k:3 + k + H]
            t = [X(k - 2) * wb[c, di, k] for k in range(5)]
            pe = ((t[0], t[1]), (t[2], t[3]), (t[4], zero))
            po = ((zero, t[0]), (t[1], t[2]), (t[3], t[4]))
            for (ea, eb), (oa, ob) in zip(pe, po):
                acc = (acc + torch.where(even, ea, oa)) + torch.where(even, eb, ob)
    return (acc + (bias.float() if bias is not None else 0.0)).to(BF)


def mfma_standin(x, w, bias):
    """csrc/proj_conv_mfma.hip in f32 for one sample: P_ds = chain over the layers of the kernel row's five products (one rounded add each),
    then v = bias + P_0[s - 2] + P_1[s - 1] + ... + P_4[s + 2] left to right"""
    C, S, H = x.shape
    wb = w.to(BF).float().view(C, 5, 5)
    xp = F.pad(x.float(), (2, 2, 2, 2))
    v = torch.zeros((S, H)) + (bias.float() if bias is not None else 0.0)
    for ds in range(5):
        acc = torch.zeros((S, H))
        for c in range(C):
            for k in range(5):
                acc = acc + xp[c, ds:ds + S, k:k + H] * wb[c, ds, k]
        v = v + acc
    return v.to(BF)


@pytest.mark.parametrize("kind", R.CONV_KINDS)
@pytest.mark.parametrize("C", [1, 8, 37, 64])
def test_conv_standins_stay_inside_the_allowance(kind, C):
    B, S, H = 2, 19, 40
    x, w, bias = R.conv_operands(kind, B, C, S, H, gen(10 + C))
    ref = R.ConvRef(x, w)
    shares = {}
    for name, fn, forms in (("valu", valu_standin, ("valu1", "valu2")), ("mfma", mfma_standin, ("mfma_pair", "mfma_pipe", "mfma_rb2"))):
        for b in (bias, None):
            y = torch.stack([fn(x[z], w, b) for z in range(B)])
            for form in forms:
                s = ref.check(f"{name} stand-in {kind} C={C}", y, form, b)
                assert s <= 1.0
                shares[form] = max(shares.get(form, 0.0), s)
    print(f"\n  {kind} C={C}: share of the f32 allowance used by the stand-ins: " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()))
    if kind == "cancel" and C > 1:
        want, bound, d = R.conv5x5_expect(x[0], w, bias, "mfma_pipe")
        inner = (want[2:-2, 2:-2].abs() / (d[2:-2, 2:-2] / (R.conv5x5_depth("mfma_pipe", C) * R.U_F32))).median()
        assert float(inner) < 0.05                   # |want| << sum|x w| inside the plane


def layer_mean_standin(x, scale):
    B, C = x.shape[:2]
    acc = torch.zeros(x[:, 0].shape)
    for c in range(C):
        acc = acc + (x[:, c].float() * scale[c] if scale is not None else x[:, c].float())
    return (acc * (torch.tensor(1.0) / torch.tensor(float(C)))).to(BF)


def seq_mean_standin(x):
    acc = torch.zeros(x[:, 0].shape)
    for s in range(x.shape[1]):
        acc = acc + x[:, s]
    return acc / torch.tensor(float(x.shape[1]))


@pytest.mark.parametrize("C", [1, 25, 64])
def test_mean_standins_stay_inside_the_allowance(C):
    x = (3.0 * torch.randn((2, C, 5, 24), generator=gen(20))).to(BF)
    sc = torch.randn(C, generator=gen(21))
    for scale in (sc, None):
        s = R.check_layer_mean("layer_mean stand-in", x, scale, layer_mean_standin(x, scale))
        assert s <= 1.0
        print(f"\n  layer_mean C={C} scale={scale is not None}: share {s:.3f}")
    for B, S, N in ((1, 1, 1), (2, 12, 768), (3, 7, 257)):
        xs = torch.randn((B, S, N), generator=gen(22))
        s = R.check_seq_mean("seq_mean stand-in", xs, seq_mean_standin(xs))
        assert s <= 1.0
        print(f"  seq_mean {(B, S, N)}: share {s:.3f}")
    # a mean that rounds its sum to bf16 before the scaling, and a sequence mean that misses its last row, are rejected
    if C == 25:                                          # (C = 64: the division is exact and the second rounding changes nothing)
        bad =(x.float().sum(1).to(BF).float() / C).to(BF)
        with pytest.raises(AssertionError, match=r"layer_mean: \d+ rows over the bound .* sample \d, row \(token\) \d"):
            R.check_layer_mean("layer_mean", x, None, bad)
    xs = torch.randn((3, 7, 257), generator=gen(23))
    bad = seq_mean_standin(xs)
    bad[2, 256] = xs[2, :6, 256].sum() / 7
    assert rel_l2(bad, xs.mean(1)) > R.OLD_SEQ_MEAN_REL_L2          # (this one the old check would have seen -- had it run N % 256 != 0)
    with pytest.raises(AssertionError, match=r"sample 2, row \(token\) 0, cols 256..511 \(col 256\)"):
        R.check_seq_mean("seq_mean", xs, bad)


# ---------------------------------------------------------------------------------------------------------------- planted faults
def good_output(x, w, bias):
    """a correct kernel's output: f32 conv on the bf16 taps, rounded once"""
    return F.conv2d(x.float(), wb_of(w), bias, padding=2)[:, 0].to(BF)


def old_checks_pass(out, x, w, bias):
    """the whole-tensor checks of tests/test_ops_gpu.py: (the matrix-core test's, the VALU test's)"""
    ref_b = F.conv2d(x.float(), wb_of(w), bias, padding=2)[:, 0]
    ref = F.conv2d(x.float(), w.view(1, -1, 5, 5), bias, padding=2)[:, 0]
    return (rel_l2(out, ref_b) < R.OLD_MFMA_REL_L2 and rel_l2(out, ref) < R.OLD_VALU_REL_L2), rel_l2(out, ref) < R.OLD_VALU_REL_L2


@pytest.fixture(scope="module")
def mfma_case():
    B, C, S, H = 1, 16, 192, 2048
    x, w, bias = R.conv_operands("random", B, C, S, H, gen(31))
    good = good_output(x, w, bias)
    ref = R.ConvRef(x, w)
    ref.check("no fault", good, "mfma_pipe", bias)
    assert old_checks_pass(good, x, w, bias) == (True, True)
    return x, w, bias, good, ref


def test_fault_right_halo_chunk_of_one_layer_read_as_zero(mfma_case):
    """tile (row block 2, column block 3) of the one-row-block MFMA forms: chunk 33 (columns h0 + 256 .. h0 + 263) of layer 5 never staged"""
    x, w, bias, good, ref = mfma_case
    c, s0, h0 = 5, 24, 768
    only = torch.zeros_like(x)
    only[0, c, :, h0 + 256:h0 + 264] = x[0, c, :, h0 + 256:h0 + 264]
    lost = F.conv2d(only.float(), wb_of(w), padding=2)[0, 0]
    v = F.conv2d(x.float(), wb_of(w), bias, padding=2)[0, 0]
    v[s0:s0 + 12, h0:h0 + 256] -= lost[s0:s0 + 12, h0:h0 + 256]
    bad = v.to(BF)[None]
    assert int((bad != good).sum()) > 0
    assert old_checks_pass(bad, x, w, bias)[0]
    with pytest.raises(AssertionError, match=r"form mfma_pipe, sample 0, output row (2[4-9]|3[0-5]), column 102[23] \(row block 2: rows 24..35, .*"
                                             r"column block 3: columns 768..1023\)"):
        ref.check("halo chunk", bad, "mfma_pipe", bias)


def test_fault_last_row_of_a_row_block_misses_kernel_row_4(mfma_case):
    """output row s0 + 11 pulls kernel row 4 from DPP lane 15: one lane's four columns of row block 3 get nothing from it"""
    x, w, bias, good, ref = mfma_case
    s, h = 36 + 11, 512 + 16 * 5 + 4 * 2
    w4 = torch.zeros_like(w).view(-1, 5, 5)
    w4[:, 4] = w.view(-1, 5, 5)[:, 4]
    lost = F.conv2d(x.float(), wb_of(w4.reshape(-1, 25)), padding=2)[0, 0]
    v = F.conv2d(x.float(), wb_of(w), bias, padding=2)[0, 0]
    v[s, h:h + 4] -= lost[s, h:h + 4]
    bad = v.to(BF)[None]
    assert old_checks_pass(bad, x, w, bias)[0]
    with pytest.raises(AssertionError, match=r"form mfma_pipe, sample 0, output row 47, column 60[0-3] \(row block 3: rows 36..47, row 11 of it; "
                                             r"column block 2: columns 512..767\)"):
        ref.check("kernel row 4", bad, "mfma_pipe", bias)
    # the same element named in the two-row-block form's blocks
    with pytest.raises(AssertionError, match=r"form mfma_rb2, .* \(row block 1: rows 24..47, row 23 of it"):
        ref.check("kernel row 4", bad, "mfma_rb2", bias)


def test_fault_second_stream_first_row_takes_its_neighbours_ring_slot():
    """the two-stream VALU kernel at S = 1361: the last block's second stream holds ONE row (1360); it stores the ring slot of output row
    1361 -- kernel rows 0 .. 3 of the NEXT output row -- in the ragged column block (columns 1024 .. 1031) of sample 1"""
    B, C, S, H = 2, 3, 1361, 1032
    assert R.valu_form(B, S, H) == "valu2"
    x, w, bias = R.conv_operands("random", B, C, S, H, gen(32))
    good = good_output(x, w, bias)
    ref = R.ConvRef(x, w)
    ref.check("no fault", good, "valu2", bias)
    w03 = w.clone().view(C, 5, 5)
    w03[:, 4] = 0.0
    nxt = F.conv2d(F.pad(x[1:2, :, S - 8:].float(), (0, 0, 0, 1)), wb_of(w03.reshape(C, 25)), bias, padding=2)[0, 0, -1]      # "output row" S
    bad = good.clone()
    bad[1, S - 1, 1024:] = nxt[1024:].to(BF)
    assert old_checks_pass(bad, x, w, bias)[1]
    with pytest.raises(AssertionError, match=r"form valu2, sample 1, output row 1360, column 10(2[4-9]|3[01]) \(row block 42: rows 1344..1375, row "
                                             r"16 of it; column block 2: columns 1024..1535\)"):
        ref.check("ring slot", bad, "valu2", bias)


def test_fault_table_entry_off_by_one_tap():
    w = torch.randn((37, 25), generator=gen(33)) / 30
    table = R.pack_expect(w)
    R.check_table("pack", table, w)
    c, ds, g, n, j = 3, 2, 1, 4, 3                     # tap 8 g + j - n - 6 = 1
    assert (g, n, j) not in R.OLD_TABLE_ENTRIES
    bad = table.clone()
    bad[c, ds, n + 16 * g, j] = w.to(BF).view(37, 5, 5)[c, ds, 2]
    # the old check: seven (g, n, j) per (layer, kernel row)
    t, wb = bad.float().view(37, 5, 4, 16, 8), w.to(BF).float().view(37, 5, 5)
    for gi, ni, ji in R.OLD_TABLE_ENTRIES:
        dh = 8 * gi + ji - ni - 6
        assert torch.equal(t[:, :, gi, ni, ji], wb[:, :, dh] if 0 <= dh <= 4 else torch.zeros(37, 5))
    with pytest.raises(AssertionError, match=r"1 table entries differ; first at layer 3, kernel row 2, lane 20 \(n=4, g=1\), j=3 \(tap 1\)"):
        R.check_table("pack", bad, w)


def test_fault_last_row_of_a_sample_unwritten_and_a_write_behind_the_output():
    """The old tests let the launch allocate its output: an unwritten row then holds whatever the allocator's block held -- after an earlier
    call of the same test, the right values.  In a poisoned buffer it still holds the sentinel."""
    B, C, S, H = 2, 3, 6, 64
    x, w, bias = R.conv_operands("random", B, C, S, H, gen(34))
    good = good_output(x, w, bias)
    stale = good.clone()                               # the block as the previous identical call left it; this launch writes every row but
    stale[:, :S - 1] = good[:, :S - 1]                 # the last, which keeps the earlier call's values
    assert old_checks_pass(stale, x, w, bias) == (True, True)
    guard, off = 2 * H, 2
    buf = R.poison_(torch.empty(guard + off + B * S * H + guard, dtype=BF))
    y = buf[guard + off:guard + off + B * S * H].view(B, S, H)
    y.copy_(good)
    mask = R.write_mask(buf, [((B, S, H), (S * H, H, 1), guard + off)])
    R.check_conv5x5("whole", x, w, bias, y, "valu1")
    R.check_untouched("whole", buf, mask, row_len=H)
    R.poison_(y[1, S - 1])
    with pytest.raises(AssertionError, match=r"64 output elements left unwritten .* form valu1, sample 1, output row 5, column 0 "):
        R.check_conv5x5("unwritten", x, w, bias, y, "valu1")
    y.copy_(good)
    buf[guard + off + B * S * H + 3] = 1.0               # row S of the last sample
    with pytest.raises(AssertionError, match=r"1 elements outside the launch's write set were written"):
        R.check_untouched("behind", buf, mask, row_len=H)
    # NaN fails
    y.copy_(good)
    y[0, 2, 5] = float("nan")
    with pytest.raises(AssertionError, match=r"sample 0, output row 2, column 5 "):
        R.check_conv5x5("nan", x, w, bias, y, "valu1")
