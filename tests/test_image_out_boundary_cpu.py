"""The extension header abi/backend/x2i_image_out.h against its binding x2i_amd/image_out_binding.py, the built library, the headers
under include/ and INTEGRATION.md (no GPU), in the way of tests/test_image_rows_boundary_cpu.py.  Also the entry points' argument checks,
which need no GPU, the binding's refusals, and the build's dependency on the new directory."""
import ctypes as C
import glob
import os

import pytest
import torch

from tests import headers

HEADER = os.path.join(headers.ROOT, "abi", "backend", "x2i_image_out.h")
NAMES = {"x2i_latents_to_vae", "x2i_image_to_u8"}      # written out, so that a renamed export fails


def test_header_matches_its_binding_and_the_library_exports_it():
    from x2i_amd import _lib, image_binding as ib, image_out_binding as iob, image_rows_binding as irb, image_tiles_binding as itb, ops
    want = headers.header_prototypes(HEADER)
    assert set(want) == set(iob._EXPORTS) == NAMES
    assert len(want["x2i_latents_to_vae"]) == 10 and len(want["x2i_image_to_u8"]) == 9
    for name, args in want.items():
        assert len(iob._EXPORTS[name]) == len(args), name
        for i, (got, exp) in enumerate(zip(iob._EXPORTS[name], args)):
            assert got == exp, "%s: argument %d is %s in the binding, %s in the header" % (name, i, got.__name__, exp.__name__)
        assert args[-1] == C.c_void_p                  # the stream comes last
    assert want["x2i_latents_to_vae"][7:9] == [C.c_float, C.c_float]       # scaling_factor and shift_factor travel as float
    lib = iob.load()
    for name in want:
        assert hasattr(lib, name) and getattr(lib, name).argtypes == iob._EXPORTS[name] and getattr(lib, name).restype is C.c_int
    base = headers.header_names(headers.include("x2i.h"))
    assert len(base) == 80                             # x2i.h still has its 80 names
    for other in (base, set(_lib._EXPORTS), set(ib._EXPORTS), set(itb._EXPORTS), set(irb._EXPORTS)):
        assert not (other & NAMES)
    assert not any(hasattr(ops, n) for n in ("latents_to_vae", "image_to_u8"))
    text = open(HEADER).read()
    assert '#include "../../include/x2i.h"' in text and "Everything x2i.h says holds here" in text
    assert "NaN gives 0" in text and "one\n * defined extension" in text


def test_no_other_header_declares_the_names_and_the_new_directory_holds_one_header():
    for path in glob.glob(headers.include("**/*.h"), recursive=True):
        assert not (headers.header_names(path) & NAMES), path
    assert len(glob.glob(headers.include("**/*.h"), recursive=True)) == 19      # include/ is as it was
    assert sorted(os.listdir(os.path.join(headers.ROOT, "abi"))) == ["backend"]
    assert sorted(os.listdir(os.path.join(headers.ROOT, "abi", "backend"))) == ["x2i_image_out.h"]
    assert os.path.exists(os.path.join(headers.ROOT, "x2i_amd", "image_out_binding.py"))
    assert not os.path.exists(os.path.join(headers.ROOT, "x2i_amd", "image_out_ops.py"))
    assert len(glob.glob(os.path.join(headers.ROOT, "x2i_amd", "*_ops.py"))) == 13


def test_integration_md_names_the_header_and_the_entry_points():
    md = open(os.path.join(headers.ROOT, "INTEGRATION.md")).read()
    assert "Extension header `abi/backend/x2i_image_out.h`" in md
    assert all("`%s`" % n in md for n in NAMES)


def test_the_build_tracks_headers_under_abi(monkeypatch):
    from x2i_amd import build
    seen = []
    real = os.path.getmtime
    monkeypatch.setattr(build.os.path, "getmtime", lambda p: seen.append(os.path.realpath(p)) or real(p))
    build._newest_header()
    assert os.path.realpath(HEADER) in seen and os.path.realpath(headers.include("x2i.h")) in seen
    assert os.path.exists(os.path.join(build.CSRC, "image_out.hip"))


def test_a_stale_library_is_reported_with_the_headers_path(monkeypatch):
    from x2i_amd import _lib, image_out_binding as iob

    class Stale:
        pass

    monkeypatch.setattr(_lib, "load", lambda: Stale)
    with pytest.raises(_lib.X2IError, match=r"does not export x2i_latents_to_vae \(abi/backend/x2i_image_out.h\)"):
        _lib.extension("backend/x2i_image_out.h", iob._EXPORTS, root="abi")()


FAKE, ODD = C.c_void_p(0x1000), C.c_void_p(0x1002)


def _lat(lib, **kw):
    """x2i_latents_to_vae on never-dereferenced pointers: two 128 x 128 latents of 16 channels unless kw says otherwise"""
    d = dict(lat=FAKE, ld=64, out=FAKE, B=2, h=128, w=128, Cz=16, sf=0.3611, sh=0.1159, st=None)
    d.update(kw)
    return lib.x2i_latents_to_vae(*[d[k] for k in ("lat", "ld", "out", "B", "h", "w", "Cz", "sf", "sh", "st")])


def _u8(lib, **kw):
    """x2i_image_to_u8 on never-dereferenced pointers: two 1024 x 1024 images at dense pitches unless kw says otherwise"""
    d = dict(y=FAKE, ldy=4, out=FAKE, ip=3 * 1024 * 1024, rp=3 * 1024, B=2, H=1024, W=1024, st=None)
    d.update(kw)
    return lib.x2i_image_to_u8(*[d[k] for k in ("y", "ldy", "out", "ip", "rp", "B", "H", "W", "st")])


def test_latents_to_vae_validates_its_arguments_without_a_gpu():
    from x2i_amd import image_out_binding as iob
    lib = iob.load()
    err = lambda: lib.x2i_last_error()      # noqa: E731
    # a valid call but for a misaligned `out` (the last check): everything before the launch passes
    assert _lat(lib, out=ODD) == -3 and b"16-byte aligned" in err()
    assert _lat(lib, out=C.c_void_p(0x1008)) == -3 and _lat(lib, lat=C.c_void_p(0x1001)) == -3 and b"2-byte aligned" in err()
    assert _lat(lib, lat=None) == -1 and b"null" in err() and _lat(lib, out=None) == -1
    assert _lat(lib, B=0) == -2 and b"B=0" in err() and _lat(lib, B=-1) == -2
    for h, w in ((127, 128), (128, 127), (0, 128), (128, 0), (1, 2), (-2, 2)):
        assert _lat(lib, h=h, w=w) == -2 and b"must be even" in err(), (h, w)
    for cz in (0, 17, -1, 64):
        assert _lat(lib, Cz=cz) == -2 and b"Cz=%d must lie in 1..16" % cz in err()
    assert _lat(lib, Cz=1, ld=4, out=ODD) == -3 and _lat(lib, Cz=4, ld=16, out=ODD) == -3 and _lat(lib, Cz=4, out=ODD) == -3
    assert _lat(lib, ld=63) == -2 and b"ld_lat=63" in err() and _lat(lib, Cz=4, ld=15) == -2 and _lat(lib, ld=0) == -2 and _lat(lib, ld=-64) == -2
    # sizes that no grid serves, and products that would wrap
    assert _lat(lib, B=1, h=46340, w=46340, out=ODD) == -3 and _lat(lib, B=1, h=46342, w=46342) == -2 and b"2^31 - 1" in err()
    assert _lat(lib, B=2 ** 31 - 1, h=2 ** 31 - 2, w=2 ** 31 - 2) == -2 and _lat(lib, B=2 ** 17, h=128, w=128) == -2
    assert _lat(lib, ld=2 ** 62) == -2 and b"63 bits" in err()
    # the scalars: a reciprocal of 0, or anything not finite, would fill the decoder's input with inf / NaN silently
    for bad in (dict(sf=0.0), dict(sf=-0.0), dict(sf=float("inf")), dict(sf=float("nan")), dict(sh=float("nan")), dict(sh=float("-inf"))):
        assert _lat(lib, **bad) == -1 and b"finite" in err(), bad
    assert _lat(lib, sf=-0.5, sh=0.0, out=ODD) == -3 and _lat(lib, sf=1e-30, sh=-3e38, out=ODD) == -3


def test_image_to_u8_validates_its_arguments_without_a_gpu():
    from x2i_amd import image_out_binding as iob
    lib = iob.load()
    err = lambda: lib.x2i_last_error()      # noqa: E731
    # a valid call but for a misaligned `y` (the last check): everything before the launch passes
    assert _u8(lib, y=ODD) == -3 and b"8-byte aligned" in err() and _u8(lib, y=C.c_void_p(0x1004)) == -3
    assert _u8(lib, y=ODD, out=C.c_void_p(0x1003)) == -3       # out needs no alignment: still the y check that refuses
    assert _u8(lib, y=None) == -1 and b"null" in err() and _u8(lib, out=None) == -1
    assert _u8(lib, B=0) == -2 and _u8(lib, H=0) == -2 and _u8(lib, W=0) == -2 and b"W=0" in err() and _u8(lib, W=-4) == -2
    for ldy in (0, 3, 5, 6, 16, -4):
        assert _u8(lib, ldy=ldy) == -2 and b"ldy=%d must be 4 or 8" % ldy in err()
    assert _u8(lib, ldy=8, y=ODD) == -3
    assert _u8(lib, rp=3 * 1024 - 1) == -2 and b"row_pitch=3071" in err() and _u8(lib, rp=0) == -2 and _u8(lib, rp=-3072) == -2
    assert _u8(lib, rp=3 * 1024 + 1, ip=1023 * 3073 + 3072, y=ODD) == -3            # an unaligned pitch, the tightest image pitch
    assert _u8(lib, rp=3 * 1024 + 1, ip=1023 * 3073 + 3071) == -2 and b"image_pitch" in err()
    assert _u8(lib, ip=3 * 1024 * 1024 - 1) == -2 and _u8(lib, ip=0) == -2 and _u8(lib, ip=-1) == -2
    assert _u8(lib, H=1, ip=3072, y=ODD) == -3 and _u8(lib, H=1, ip=3071) == -2 and _u8(lib, B=1, H=1, W=1, rp=3, ip=3, y=ODD) == -3
    # no product that could wrap, no grid beyond 2^31 - 1 blocks' worth of lanes
    assert _u8(lib, rp=2 ** 62, ip=2 ** 63 - 1) == -2
    assert _u8(lib, B=2 ** 20, H=2 ** 20, W=4, rp=12, ip=12 * 2 ** 20) == -2 and b"2^31 - 1" in err()
    assert _u8(lib, B=2, ip=2 ** 62, y=ODD) == -2 and b"63 bits" in err()


def test_the_binding_refuses_what_the_launcher_refuses(monkeypatch):
    from x2i_amd import image_out_binding as iob
    X = iob.X2IError
    lat, out = torch.zeros(2, 3 * 5, 64, dtype=torch.bfloat16), torch.zeros(2, 6, 10, 64, dtype=torch.bfloat16)
    args = iob._latents_args(lat, 6, 10, 16, 0.3611, 0.1159, out)
    assert len(args) == 9 and args[1] == 64 and args[3:7] == (2, 6, 10, 16) and args[7:] == (0.3611, 0.1159)
    assert iob._latents_args(lat, 6, 10, 4, 1.0, 0.0, out)[6] == 4
    for change, msg in ((dict(h=5), "must be even"), (dict(h=8), "packed rows"), (dict(Cz=17), "1..16"), (dict(Cz=0), "1..16"),
                        (dict(lat=lat[:, :, :32]), "contiguous"), (dict(lat=lat[:, :, :32].contiguous()), "hold 4 Cz"),
                        (dict(lat=lat.float()), "bfloat16"), (dict(out=out[:, :, :, :32]), "contiguous"), (dict(out=out[:1]), r"out must be \[2, 6, 10, 64\]"),
                        (dict(lat=lat[0]), "packed rows")):
        d = dict(lat=lat, h=6, w=10, Cz=16, out=out)
        d.update(change)
        with pytest.raises(X, match=msg):
            iob._latents_args(d["lat"], d["h"], d["w"], d["Cz"], 0.3611, 0.1159, d["out"])
    y, buf = torch.zeros(2, 3, 5, 4, dtype=torch.bfloat16), torch.zeros(2 * 3 * 20 + 7, dtype=torch.uint8)
    assert iob._u8_args(y, buf, 60, 20, 7)[1:2] + iob._u8_args(y, buf, 60, 20, 7)[3:] == (4, 60, 20, 2, 3, 5)
    assert iob._u8_args(y, buf, 60, 20, 7)[2].value == buf.data_ptr() + 7
    for change, msg in ((dict(off=13), "need"), (dict(rp=14), "at least 3 W"), (dict(ip=54), "at least"), (dict(off=-1), "not negative"),
                        (dict(y=y[..., :3]), "contiguous"), (dict(y=torch.zeros(2, 3, 5, 6, dtype=torch.bfloat16)), "4 or 8"),
                        (dict(y=y.float()), "bfloat16"), (dict(buf=buf.to(torch.int8)), "uint8"), (dict(buf=buf[::2]), "uint8 buffer")):
        d = dict(y=y, buf=buf, ip=60, rp=20, off=7)
        d.update(change)
        with pytest.raises(X, match=msg):
            iob._u8_args(d["y"], d["buf"], d["ip"], d["rp"], d["off"])
    with pytest.raises(X, match="must live on the GPU"):       # no fallback: CPU tensors are refused by name
        iob.image_to_u8(y)
    with pytest.raises(X, match="must live on the GPU"):
        iob.latents_to_vae(lat, 6, 10, 16, 0.3611, 0.1159)


def test_the_harness_flag_and_the_writer_need_no_gpu(tmp_path):
    from x2i_amd.image_out import ImageWriter
    from x2i_amd.infer import harness as H
    p = H.build_parser("qwenvl")
    assert p.parse_args(["--synthetic"]).hip_image_out is False
    assert p.parse_args(["--synthetic", "--decode", "--hip_image_out"]).hip_image_out is True
    assert "--hip_image_out" in p.format_help() and "same .jpg bytes" in " ".join(p.format_help().split())
    for family in ("internvl", "minicpm"):
        assert H.build_parser(family).parse_args(["--hip_image_out"]).hip_image_out is True

    class Ticket:       # a host-only stand-in: what the writer needs of image_out.Ticket
        def __init__(self, arrays):
            self._arrays, self.released, self.waited = arrays, False, 0

        def arrays(self):
            self.waited += 1
            return self._arrays

        def release(self):
            self.released = True

    import numpy as np
    from PIL import Image
    rng = np.random.default_rng(0)
    imgs = [rng.integers(0, 256, size=(24, 40, 3), dtype=np.uint8) for _ in range(3)]
    w = ImageWriter()
    t1, t2 = Ticket(imgs[:2]), Ticket(imgs[2:])
    w.put(t1, [str(tmp_path / "a.jpg"), str(tmp_path / "b.png")])
    w.put(t2, [str(tmp_path / "c.jpg")])
    w.flush()
    assert t1.released and t2.released and not w.failed
    for name, a in zip(("a.jpg", "b.png", "c.jpg"), imgs):
        Image.fromarray(a).save(str(tmp_path / ("want_" + name)))
        assert (tmp_path / name).read_bytes() == (tmp_path / ("want_" + name)).read_bytes()
    # a path that cannot be written: the exception comes out of flush(), what was queued behind it is released untouched, put refuses
    bad, later = Ticket(imgs[:1]), Ticket(imgs[1:2])
    w.put(bad, [str(tmp_path / "no_such_directory" / "x.jpg")])
    w.put(later, [str(tmp_path / "later.jpg")])
    with pytest.raises(OSError):
        w.flush()
    assert bad.released and later.released and later.waited == 0 and not (tmp_path / "later.jpg").exists() and not w.failed
    # the harness: after a failed save nothing more is enqueued, and what is raised is the writer's own exception
    class Back:
        submits = 0

        def submit(self, *a):
            Back.submits += 1
            return Ticket(imgs[:1])

    hs = H.Harness.__new__(H.Harness)
    hs.image_out, hs.writer = Back(), w
    hs._save_hip(None, 24, 40, [str(tmp_path / "first.jpg")])
    hs.flush_outputs()
    assert Back.submits == 1 and (tmp_path / "first.jpg").exists()
    hs._save_hip(None, 24, 40, [str(tmp_path / "no_such_directory" / "z.jpg")])
    w._q.join()
    assert w.failed
    with pytest.raises(OSError):
        hs._save_hip(None, 24, 40, [str(tmp_path / "never.jpg")])
    assert Back.submits == 2 and not (tmp_path / "never.jpg").exists() and not w.failed
    w.put(Ticket(imgs[:1]), [str(tmp_path / "again.jpg")])     # usable again once the failure was raised
    w.close()
    assert (tmp_path / "again.jpg").exists() and not w._thread.is_alive()
    with pytest.raises(RuntimeError, match="closed"):
        w.put(Ticket(imgs[:1]), [str(tmp_path / "closed.jpg")])
