"""The image back end on the GPU (abi/backend/x2i_image_out.h, x2i_amd/image_out.py): both kernels bit for bit against the torch
expressions they replace, run on the device, and against the numpy restatements (tests/image_out_ref.py) for every bf16 bit pattern;
guard bytes; decode_to_uint8 against postprocess(decode(...)); the ring, the writer and the files; graph capture; the harness flag."""
import glob
import os

import numpy as np
import pytest
import torch

from tests import image_out_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLUX = (0.3611, 0.1159)
OTHER = (0.13025, 0.0609)


def _dev_bf16(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(DEV).view(torch.bfloat16)


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


# ------------------------------------------------------------------------------------------------------------- x2i_latents_to_vae
@pytest.mark.parametrize("Cz,ld", [(16, 64), (4, 16), (4, 64)])
@pytest.mark.parametrize("h,w", [(2, 2), (2, 6), (4, 2), (6, 10)])
def test_latents_to_vae_every_pattern_against_torch_on_the_device_and_the_restatement(h, w, Cz, ld):
    """All 65536 patterns laid through launches of B = 2: launch k reads the next 2 * (h / 2)(w / 2) * 4 Cz of them (the last one wraps).
    ld = 64 with Cz = 4: the 48 values behind a row's 16 are NaNs that must not be read."""
    from x2i_amd import image_out_binding as iob
    from x2i_amd.pipeline import FluxPipeline
    B, rows, used = 2, (h // 2) * (w // 2), 4 * Cz
    per = B * rows * used
    n = -(-65536 // per)
    vals = np.resize(R.ALL_BF16, n * per).reshape(n * B, rows, used)
    assert set(vals.ravel().tolist()) == set(range(65536))
    bits = np.full((n * B, rows, ld), 0x7FC1, dtype=np.uint16)
    bits[:, :, :used] = vals
    lat = _dev_bf16(bits)
    for consts in (FLUX, OTHER):
        sf, shift = consts
        out = torch.full((n * B, h, w, 64), -1, dtype=torch.int16, device=DEV).view(torch.bfloat16)
        for k in range(n):
            iob.latents_to_vae(lat[k * B:(k + 1) * B], h, w, Cz, sf, shift, out=out[k * B:(k + 1) * B])
        got = _bits(out)
        # the parent's path on the device: _unpack_latents, the bf16 divide and add, decode's zero pad and NHWC copy
        z = FluxPipeline._unpack_latents(lat[:, :, :used].contiguous(), 8 * h, 8 * w, 16)
        z = (z / sf) + shift
        x = torch.zeros((n * B, h, w, 64), device=DEV, dtype=torch.bfloat16)
        x[..., :Cz] = z.to(torch.bfloat16).permute(0, 2, 3, 1)
        want = _bits(x)
        ref = R.latents_to_vae(bits, h, w, Cz, sf, shift, device=True)
        bad = np.argwhere(got != want)
        assert bad.size == 0, "%d elements differ from torch on the device, first %s: %04x against %04x" % (
            len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
        bad = np.argwhere(got != ref)
        assert bad.size == 0, "%d elements differ from the restatement, first %s: %04x against %04x" % (
            len(bad), bad[0], got[tuple(bad[0])], ref[tuple(bad[0])])
        assert (got[..., Cz:] == 0).all()                      # pad channels: +0, every one written
        again = torch.full_like(out.view(torch.int16), -1).view(torch.bfloat16)
        iob.latents_to_vae(lat[:B], h, w, Cz, sf, shift, out=again[:B])
        assert np.array_equal(_bits(again[:B]), got[:B])       # a relaunch gives the same bits


# ---------------------------------------------------------------------------------------------------------------- x2i_image_to_u8
def _harness_expression(y):
    """harness.generate's line on the device, from the NCHW image decode returns"""
    image = y[..., :3].permute(0, 3, 1, 2).contiguous()
    return ((image.float() / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()


@pytest.mark.parametrize("ldy", [4, 8])
def test_image_to_u8_every_pattern_dense(ldy):
    from x2i_amd import image_out_binding as iob
    bits = np.full((2 * 96 * 128, ldy), 0x7FC1, dtype=np.uint16)       # channels 3 .. : junk that must not show
    bits[:, :3] = np.resize(R.ALL_BF16, (2 * 96 * 128, 3))
    bits = bits.reshape(2, 96, 128, ldy)
    y = _dev_bf16(bits)
    got = iob.image_to_u8(y).cpu().numpy()
    ref = R.image_to_u8(bits)
    assert got.shape == (2, 96, 128, 3) and np.array_equal(got, ref)
    nan = R.is_nan_bf16(bits[..., :3])
    assert nan.sum() == 254 and (got[nan] == 0).all()
    want = _harness_expression(y)
    assert np.array_equal(got[~nan], want[~nan])
    assert np.array_equal(iob.image_to_u8(y).cpu().numpy(), got)


@pytest.mark.parametrize("B,H", [(1, 1), (1, 3), (2, 1), (2, 3)])
def test_image_to_u8_pitches_offsets_and_guard_bytes(B, H):
    """W x ldy x row pitch x base offset: every combination one launch into a buffer of guard bytes, compared whole.  The patterns walk
    on from launch to launch; the dense test covers all of them."""
    from x2i_amd import image_out_binding as iob
    pos, GUARD = 7919 * (B * 2 + H), 0xA5
    for W in (1, 3, 4, 5, 8, 67):
        for ldy in (4, 8):
            for extra in (0, 1, 5):
                for off in (0, 1, 2, 3):
                    rp = 3 * W + extra
                    ip = H * rp + (11 if extra else 0)
                    bits = np.full((B, H, W, ldy), 0xFFFF, dtype=np.uint16)
                    bits[..., :3] = np.resize(np.roll(R.ALL_BF16, -pos), (B, H, W, 3))
                    pos = (pos + B * H * W * 3) % 65536
                    y = _dev_bf16(bits)
                    front, size = 16 + off, 16 + off + B * ip + 16
                    buf = torch.full((size,), GUARD, dtype=torch.uint8, device=DEV)
                    iob.image_to_u8(y, out=buf, image_pitch=ip, row_pitch=rp, offset=front)
                    want = np.full(size, GUARD, dtype=np.uint8)
                    ref = R.image_to_u8(bits)
                    for n in range(B):
                        for r in range(H):
                            s = front + n * ip + r * rp
                            want[s:s + 3 * W] = ref[n, r].ravel()
                    got = buf.cpu().numpy()
                    assert np.array_equal(got, want), (W, ldy, rp, ip, off, np.nonzero(got != want)[0][:8])
                    nan = R.is_nan_bf16(bits[..., :3])
                    dense = np.stack([got[front + n * ip + r * rp:][:3 * W].reshape(W, 3) for n in range(B) for r in range(H)]).reshape(B, H, W, 3)
                    assert np.array_equal(dense[~nan], _harness_expression(y)[~nan])


# ---------------------------------------------------------------------------------------------------- decode_to_uint8, ring, writer
@pytest.fixture(scope="module")
def tiny():
    """a two-level VAE with random weights (vae_scale_factor 4: a 32 x 32 image has 16 x 16 latents), and the parent's tail around it"""
    from x2i_amd.pipeline import FluxPipeline, VaeImageProcessor
    from x2i_amd.vae import AutoencoderKL
    vae = AutoencoderKL(block_out_channels=(128, 128), layers_per_block=1, device=DEV).init_random_(11)

    def latents(B, height, width, seed):
        g = torch.Generator().manual_seed(seed)
        return (torch.randn((B, (height // 4) * (width // 4), 64), generator=g) * 1.5).to(torch.bfloat16).to(DEV)

    def parent(lat, height, width):
        x = FluxPipeline._unpack_latents(lat, height, width, 4)
        x = (x / vae.config.scaling_factor) + vae.config.shift_factor
        return VaeImageProcessor(vae_scale_factor=4).postprocess(vae.decode(x, return_dict=False)[0], output_type="pil")

    return vae, latents, parent


@pytest.mark.parametrize("height,width", [(32, 32), (48, 32)])
def test_decode_to_uint8_equals_postprocess_of_decode(tiny, height, width):
    from x2i_amd.pipeline import FluxPipeline
    vae, latents, parent = tiny
    lat = latents(2, height, width, 5)
    x = FluxPipeline._unpack_latents(lat, height, width, 4)
    x = (x / vae.config.scaling_factor) + vae.config.shift_factor
    before = vae.decode(x, return_dict=False)[0].clone()
    want = np.stack([np.asarray(p) for p in parent(lat, height, width)])
    got = vae.decode_to_uint8(lat, height, width)
    assert got.shape == (2, height, width, 3) and got.dtype == torch.uint8
    assert np.array_equal(got.cpu().numpy(), want)
    assert want.std() > 20                                     # an image, not a constant
    # decode itself: the same bits before and after the new path ran, NCHW, and the body's NHWC output behind the parent's pad and copy
    after = vae.decode(x, return_dict=False)[0]
    assert after.shape == (2, 3, height, width) and after.is_contiguous() and torch.equal(before, after)
    pad = torch.zeros((2, height // 2, width // 2, 64), device=DEV, dtype=torch.bfloat16)
    pad[..., :16] = x.permute(0, 2, 3, 1)
    assert torch.equal(vae._decode_nhwc(pad)[..., :3].permute(0, 3, 1, 2), after)
    assert torch.equal(vae.decode(x).sample, after)
    # the A/B form of conv_out leaves ldy = 8: the same pixels
    vae.narrow_conv_out = False
    try:
        assert np.array_equal(vae.decode_to_uint8(lat, height, width).cpu().numpy(), want)
    finally:
        vae.narrow_conv_out = True


def test_back_end_ring_tickets_and_writer_files(tiny, tmp_path):
    from x2i_amd.image_out import ImageBackEnd, ImageWriter
    vae, latents, parent = tiny
    back = ImageBackEnd(vae, DEV, slots=2)
    lats = [latents(2, 32, 32, 1), latents(2, 32, 32, 2), latents(2, 48, 32, 3)]
    wants = [[np.asarray(p) for p in parent(lats[0], 32, 32)], [np.asarray(p) for p in parent(lats[1], 32, 32)],
             [np.asarray(p) for p in parent(lats[2], 48, 32)]]
    t1, t2 = back.submit(lats[0], 32, 32), back.submit(lats[1], 32, 32)
    assert back.regrown == 2 and t1.shape == (2, 32, 32)
    with pytest.raises(RuntimeError, match="not released"):    # both slots hold a ticket: the third submit has nowhere to go
        back.submit(lats[2], 48, 32, timeout=0)
    with t2 as arrays:                                         # the second one first
        assert all(np.array_equal(a, w) for a, w in zip(arrays, wants[1]))
    with pytest.raises(RuntimeError, match="not released"):    # ring order: the next slot is still the first ticket's
        back.submit(lats[2], 48, 32, timeout=0)
    late = t1.arrays()                                         # consumed late: still its own pixels
    assert all(np.array_equal(a, w) for a, w in zip(late, wants[0]))
    t1.release()
    with pytest.raises(RuntimeError, match="released"):
        t1.arrays()
    t3 = back.submit(lats[2], 48, 32)                          # a larger batch: the slot is regrown
    assert back.regrown == 3
    t4 = back.submit(lats[0], 32, 32)                          # the other slot, large enough as it is
    assert back.regrown == 3
    # the writer: the files of the path without the back end, byte for byte
    writer = ImageWriter()
    names3, names4 = ["c_b0.jpg", "c_b1.jpg"], ["a_b0.jpg", "a_b1.png"]
    writer.put(t3, [str(tmp_path / n) for n in names3])
    writer.put(t4, [str(tmp_path / n) for n in names4])
    writer.flush()
    assert t3.released and t4.released
    for names, lat, hw in ((names3, lats[2], (48, 32)), (names4, lats[0], (32, 32))):
        for name, im in zip(names, parent(lat, *hw)):
            im.save(str(tmp_path / ("want_" + name)))
            assert (tmp_path / name).read_bytes() == (tmp_path / ("want_" + name)).read_bytes(), name
    # an unwritable path: flush() raises it, the ticket behind it is released without a wait, and the ring goes on serving
    bad, behind = back.submit(lats[0], 32, 32), back.submit(lats[1], 32, 32)
    waited = []
    real = behind.arrays
    behind.arrays = lambda: waited.append(1) or real()
    writer.put(bad, [str(tmp_path / "missing" / "x.jpg"), str(tmp_path / "missing" / "y.jpg")])
    writer.put(behind, [str(tmp_path / "behind_b0.jpg"), str(tmp_path / "behind_b1.jpg")])
    with pytest.raises(OSError):
        writer.flush()
    assert bad.released and behind.released and not waited and not (tmp_path / "behind_b0.jpg").exists()
    with back.submit(lats[1], 32, 32) as arrays:
        assert all(np.array_equal(a, w) for a, w in zip(arrays, wants[1]))
    writer.close()


def test_both_kernels_inside_a_captured_graph():
    from x2i_amd import image_out_binding as iob
    rng = np.random.default_rng(9)
    lat = _dev_bf16(rng.integers(0, 65536, size=(2, 3 * 5, 64), dtype=np.uint16))
    ybits = rng.integers(0, 65536, size=(2, 3, 67, 4), dtype=np.uint16)
    y = _dev_bf16(ybits)
    eager_x = iob.latents_to_vae(lat, 6, 10, 16, *FLUX)
    eager_u = iob.image_to_u8(y)
    gx = torch.full_like(eager_x.view(torch.int16), -1).view(torch.bfloat16)
    gu = torch.full((2 * 3 * 67 * 3,), 0xA5, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        iob.latents_to_vae(lat, 6, 10, 16, *FLUX, out=gx)
        iob.image_to_u8(y, out=gu)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(gx), _bits(eager_x)) and np.array_equal(_bits(gx), R.latents_to_vae(_bits(lat), 6, 10, 16, *FLUX))
    assert np.array_equal(gu.cpu().numpy().reshape(2, 3, 67, 3), eager_u.cpu().numpy())
    assert np.array_equal(eager_u.cpu().numpy(), R.image_to_u8(ybits))


# ---------------------------------------------------------------------------------------------------------------------- end to end
def test_the_harness_writes_the_same_files_with_and_without_the_flag(tmp_path):
    from x2i_amd.infer import inference_qwenvl
    common = ["--synthetic", "--decode", "--task", "text2image", "--height", "256", "--width", "256", "--batch", "2", "--qwen_size", "3b",
              "--num_steps", "2", "--seed", "5"]
    inference_qwenvl.main(common + ["--outputs", str(tmp_path / "plain")])
    inference_qwenvl.main(common + ["--outputs", str(tmp_path / "hip"), "--hip_image_out"])
    plain = sorted(os.path.relpath(p, str(tmp_path / "plain")) for p in glob.glob(str(tmp_path / "plain" / "**" / "*.*"), recursive=True))
    hip = sorted(os.path.relpath(p, str(tmp_path / "hip")) for p in glob.glob(str(tmp_path / "hip" / "**" / "*.*"), recursive=True))
    assert plain == hip and len(plain) == 12 and all(p.endswith(".jpg") for p in plain)        # six prompts, two images each
    for p in plain:
        assert (tmp_path / "plain" / p).read_bytes() == (tmp_path / "hip" / p).read_bytes(), p
    from PIL import Image
    assert Image.open(str(tmp_path / "hip" / plain[0])).size == (256, 256)
