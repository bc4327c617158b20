"""The extension header include/frontend/tiles/x2i_image_tiles.h against its binding x2i_amd/image_tiles_binding.py, the built library,
the other headers and INTEGRATION.md (no GPU), in the way of tests/test_image_boundary_cpu.py.  Also the entry point's argument checks,
which need no GPU, the binding's refusals against the launcher's for the same sizes, and the build's dependency on the new directory."""
import ctypes as C
import glob
import os

import pytest
import torch

from tests import headers

HEADER = "frontend/tiles/x2i_image_tiles.h"
NAMES = {"x2i_image_tiles"}      # written out, so that a renamed export fails


def test_header_matches_its_binding_and_the_library_exports_it():
    from x2i_amd import _lib, image_binding as ib, image_tiles_binding as itb, ops
    want = headers.header_prototypes(headers.include(HEADER))
    assert set(want) == set(itb._EXPORTS) == NAMES
    for name, args in want.items():
        assert len(itb._EXPORTS[name]) == len(args), name
        for i, (got, exp) in enumerate(zip(itb._EXPORTS[name], args)):
            assert got == exp, "%s: argument %d is %s in the binding, %s in the header" % (name, i, got.__name__, exp.__name__)
        assert args[-1] == C.c_void_p                  # the stream comes last
    lib = itb.load()
    for name in want:
        assert hasattr(lib, name) and getattr(lib, name).argtypes == itb._EXPORTS[name] and getattr(lib, name).restype is C.c_int
    base = headers.header_names(headers.include("x2i.h"))
    assert not (base & NAMES) and not (set(_lib._EXPORTS) & NAMES) and not (set(ib._EXPORTS) & NAMES)
    assert not any(hasattr(ops, n) for n in ("image_tiles", "tiles"))
    assert '#include "../../x2i.h"' in open(headers.include(HEADER)).read()


def test_no_other_header_declares_the_name_and_the_new_directory_holds_one_header():
    others = (glob.glob(headers.include("x2i_*.h")) + glob.glob(headers.include("ext/*.h")) + glob.glob(headers.include("ext/*/*.h"))
              + glob.glob(headers.include("frontend/*.h")))
    assert len(others) == 16
    for path in others:
        assert not (headers.header_names(path) & NAMES), path
    assert headers.header_names(headers.include("frontend/x2i_image.h")) == {"x2i_image_frontend"}
    assert sorted(os.path.relpath(p, headers.include("frontend")) for p in glob.glob(headers.include("frontend/*/*.h"))) == ["tiles/x2i_image_tiles.h"]
    assert os.path.exists(os.path.join(headers.ROOT, "x2i_amd", "image_tiles_binding.py"))
    assert not os.path.exists(os.path.join(headers.ROOT, "x2i_amd", "image_tiles_ops.py"))


def test_integration_md_names_the_header_and_the_entry_point():
    md = open(os.path.join(headers.ROOT, "INTEGRATION.md")).read()
    assert "Extension header `include/frontend/tiles/x2i_image_tiles.h`" in md
    assert all("`%s`" % n in md for n in NAMES)


def test_the_build_tracks_headers_under_include_frontend_tiles(monkeypatch):
    from x2i_amd import build
    path = os.path.realpath(headers.include(HEADER))
    seen = []
    real = os.path.getmtime
    monkeypatch.setattr(build.os.path, "getmtime", lambda p: seen.append(os.path.realpath(p)) or real(p))
    build._newest_header()
    assert path in seen and os.path.realpath(headers.include("frontend/x2i_image.h")) in seen
    assert os.path.realpath(os.path.join(build.CSRC, "image_passes.h")) in seen


def test_a_stale_library_is_reported_with_the_headers_path(monkeypatch):
    from x2i_amd import _lib, image_tiles_binding as itb

    class Stale:
        pass

    monkeypatch.setattr(_lib, "load", lambda: Stale)
    with pytest.raises(_lib.X2IError, match=r"does not export x2i_image_tiles \(include/frontend/tiles/x2i_image_tiles.h\)"):
        _lib.extension(HEADER, itb._EXPORTS)()


ORDER = ("frames", "fp", "rp", "n", "iw", "ih", "ow", "oh", "tw", "th", "hb", "hc", "hk", "vb", "vc", "vk", "lut", "out", "ofs", "ots", "ors",
         "layout", "bf16", "st")


def _call(lib, **kw):
    """x2i_image_tiles on never-dereferenced pointers: 1280 x 720 -> 1470 x 812 as 3 x 2 strip crops of 490 x 406 (35 x 29 patches), two
    frames, unless kw says otherwise"""
    fake = C.c_void_p(0x1000)
    rs = 14 * (35 * 29 + 2)
    d = dict(frames=fake, fp=3 * 1280 * 720, rp=3 * 1280, n=2, iw=1280, ih=720, ow=1470, oh=812, tw=490, th=406, hb=fake, hc=fake, hk=5, vb=fake,
             vc=fake, vk=5, lut=fake, out=fake, ofs=6 * 42 * rs + 3, ots=42 * rs, ors=rs, layout=0, bf16=0, st=None)
    d.update(kw)
    return lib.x2i_image_tiles(*[d[k] for k in ORDER])


def test_the_entry_point_validates_its_arguments_without_a_gpu():
    from x2i_amd import image_binding as ib, image_tiles_binding as itb
    lib = itb.load()
    err = lambda: lib.x2i_last_error()      # noqa: E731
    call = lambda **kw: _call(lib, **kw)    # noqa: E731
    assert ib.ksize(1280, 1470) == 5 and ib.ksize(720, 812) == 5
    # a valid call but for a misaligned `out` (the last check): everything before the launch passes
    assert call(out=C.c_void_p(0x1002)) == -3 and b"element size" in err()
    for k in ("frames", "lut", "out"):
        assert call(**{k: None}) == -1 and b"null" in err()
    assert call(n=0) == -2 and b"n=0" in err() and call(n=65536) == -2
    assert call(iw=0) == -2 and b"in_w=0" in err() and call(ih=65536) == -2 and b"in_h=65536" in err()
    assert call(tw=489) == -2 and b"tile_w=489" in err() and call(tw=0) == -2 and call(tw=994) == -2 and b"14..980" in err()
    assert call(th=405) == -2 and b"tile_h=405" in err() and call(th=0) == -2 and call(th=994) == -2
    assert call(ow=1469) == -2 and b"out_w=1469 must be 1..12 times tile_w=490" in err() and call(ow=0) == -2
    assert call(ow=13 * 490) == -2 and b"out_w=6370" in err() and call(oh=13 * 406) == -2 and b"out_h=5278" in err()
    assert call(oh=811) == -2 and b"out_h=811 must be 1..12 times tile_h=406" in err() and call(oh=203) == -2
    assert call(layout=2) == -1 and b"layout=2" in err() and call(layout=-1) == -1
    assert call(rp=3 * 1280 - 1) == -2 and b"row_pitch=3839" in err() and call(fp=3 * 1280 * 720 - 1) == -2 and b"frame_pitch" in err()
    assert call(hk=7) == -2 and b"hk=7" in err() and b"ksize 5" in err() and call(vk=0) == -2 and b"vk=0" in err()
    assert call(hb=None) == -1 and b"hbound" in err() and call(hc=None) == -1 and call(vb=None) == -1 and b"vbound" in err() and call(vc=None) == -1
    # an axis that does not resize takes no tables: 1470 wide in, and 812 high in
    same = dict(iw=1470, rp=3 * 1470, fp=3 * 1470 * 720)
    assert call(hk=5, **same) == -2 and b"ksize 0" in err() and call(hk=0, **same) == -1 and b"exactly where in_w != out_w" in err()
    assert call(hk=0, hb=None, hc=None, out=C.c_void_p(0x1002), **same) == -3
    assert call(ih=812, fp=3 * 1280 * 812, vk=0) == -1 and b"exactly where in_h != out_h" in err()
    # the strides of the two layouts
    rs = 14 * (35 * 29 + 2)
    assert call(ors=14 * 35 * 29 - 1) == -2 and b"out_row_stride" in err() and call(ots=42 * rs - 1) == -2 and call(ofs=6 * 42 * rs - 1) == -2
    assert call(ors=14 * 35 * 29, ots=42 * 14 * 35 * 29, ofs=6 * 42 * 14 * 35 * 29, out=C.c_void_p(0x1002)) == -3          # the tight strides
    planar = dict(layout=1, ors=493, ots=3 * 406 * 493 + 1, ofs=6 * (3 * 406 * 493 + 1) + 5)
    assert call(out=C.c_void_p(0x1002), **planar) == -3
    assert call(**dict(planar, ors=489)) == -2 and b"layout 1" in err() and call(**dict(planar, ots=3 * 406 * 493 - 1)) == -2
    assert call(**dict(planar, ofs=6 * (3 * 406 * 493 + 1) - 1)) == -2 and b"out_frame_stride" in err()
    assert call(ors=493) == -2          # a planar row stride under the strip layout
    for k in ("hb", "hc", "vb", "vc", "lut"):
        assert call(**{k: C.c_void_p(0x1002)}) == -3 and b"4-byte aligned" in err()
    assert call(out=C.c_void_p(0x1001), bf16=1) == -3 and call(out=C.c_void_p(0x1002), bf16=1, n=0) == -2


def test_the_lds_plan_is_that_of_the_whole_resize():
    """rows come from in_h -> out_h of the WHOLE resized image, whatever the crops' height: the launcher refuses exactly the scales
    image_binding.lds_plan refuses"""
    from x2i_amd import image_binding as ib, image_tiles_binding as itb
    lib = itb.load()
    seen = set()
    for ih, gy in ((1489, 1), (1490, 1), (3000, 3), (3600, 3), (4200, 3), (4800, 3), (12000, 12), (30000, 12)):
        oh = 14 * gy
        try:
            fits = ib.lds_plan(ih, oh)[0] * 44 <= ib.LDS_BYTES
        except ib.X2IError:
            fits = False
        seen.add((gy, fits))
        rc = _call(lib, ih=ih, oh=oh, th=14, vk=ib.ksize(ih, oh), fp=3 * 1280 * ih, ors=14 * 35, ots=42 * 14 * 35, ofs=3 * gy * 42 * 14 * 35,
                   out=C.c_void_p(0x1002))
        msg = lib.x2i_last_error()
        assert (rc, b"LDS plan does not fit" in msg) == ((-3, False) if fits else (-2, True)), (ih, gy, rc, msg)
        if fits:
            assert itb.check_sizes(1280, ih, 1470, oh, 490, 14) == (3, gy)
        else:
            with pytest.raises(ib.X2IError, match="LDS plan does not fit"):
                itb.check_sizes(1280, ih, 1470, oh, 490, 14)
    assert seen == {(gy, fits) for gy in (1, 3, 12) for fits in (True, False)}


def test_the_binding_refuses_what_the_launcher_refuses(monkeypatch):
    from x2i_amd import image_binding as ib, image_tiles_binding as itb, ops
    assert itb.check_sizes(640, 480, 728, 546, 364, 546) == (2, 1) and itb.check_sizes(97, 61, 1344, 896, 448, 448) == (3, 2)
    assert itb.check_sizes(4000, 3000, 9 * 980, 980, 980, 980) == (9, 1) and itb.check_sizes(640, 480, 12 * 448, 12 * 448, 448, 448) == (12, 12)
    for args, msg in (((0, 480, 728, 546, 364, 546), "in_w=0"), ((640, 480, 728, 546, 363, 546), "tile_w=363"), ((640, 480, 728, 546, 364, 994), "tile_h=994"),
                      ((640, 480, 727, 546, 364, 546), "out_w=727 must be 1..12 times tile_w=364"), ((640, 480, 13 * 14, 14, 14, 14), "out_w=182"),
                      ((640, 480, 14, 13 * 14, 14, 14), "out_h=182 must be 1..12 times tile_h=14"), ((640, 480, 364, 546, 728, 546), "out_w=364")):
        with pytest.raises(ib.X2IError, match=msg):
            itb.check_sizes(*args)
    # the buffer checks of the tensor wrapper, on CPU tensors: the device check is taken out, no pointer is used
    monkeypatch.setattr(ops, "_req", lambda t, dtype, name: None)
    frames, lut = torch.zeros(2 * 3 * 20 * 10, dtype=torch.uint8), torch.zeros(3, 256)
    hb, hc = torch.zeros(56, 2, dtype=torch.int32), torch.zeros(56, ib.ksize(20, 56), dtype=torch.int32)
    vb, vc = torch.zeros(28, 2, dtype=torch.int32), torch.zeros(28, ib.ksize(10, 28), dtype=torch.int32)
    ok = dict(frames=frames, in_w=20, in_h=10, row_pitch=60, frame_pitch=600, n=2, out_w=56, out_h=28, tile_w=28, tile_h=14, hbound=hb, hcoef=hc,
              vbound=vb, vcoef=vc, lut=lut, out=torch.zeros(2 * 4 * 42 * 28), out_frame_stride=4 * 42 * 28, out_tile_stride=42 * 28,
              out_row_stride=28, layout=0)
    assert len(itb._tiles_args(**ok)) == 23
    assert len(itb._tiles_args(**dict(ok, layout=1, out_row_stride=28, out_tile_stride=3 * 14 * 28))) == 23
    for change, msg in ((dict(out=torch.zeros(2 * 4 * 42 * 28 - 1)), "do not fit"), (dict(out_tile_stride=42 * 28 - 1), "do not fit"),
                        (dict(out_frame_stride=4 * 42 * 28 - 1), "do not fit"), (dict(out_row_stride=27), "do not fit"),
                        (dict(frames=frames[:-1]), "frames holds"), (dict(layout=2), "layout=2"), (dict(out=torch.zeros(9408, dtype=torch.float16)), "float32 or bfloat16"),
                        (dict(hbound=None), "horizontal tables are missing"), (dict(vcoef=vc[:, :-1]), "vertical tables must be contiguous"),
                        (dict(lut=torch.zeros(3, 255)), "lut must be")):
        with pytest.raises(ib.X2IError, match=msg):
            itb._tiles_args(**dict(ok, **change))
