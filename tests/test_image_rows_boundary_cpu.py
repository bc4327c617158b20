"""The extension header include/frontend/rows/qwen/x2i_image_rows.h against its binding x2i_amd/image_rows_binding.py, the built library,
the other headers and INTEGRATION.md (no GPU), in the way of tests/test_image_tiles_boundary_cpu.py.  Also the entry point's argument
checks, which need no GPU, the binding's refusals against the launcher's for the same sizes, and the build's dependency on the new
directory."""
import ctypes as C
import glob
import os

import pytest
import torch

from tests import headers

HEADER = "frontend/rows/qwen/x2i_image_rows.h"
NAMES = {"x2i_image_rows"}      # written out, so that a renamed export fails


def test_header_matches_its_binding_and_the_library_exports_it():
    from x2i_amd import _lib, image_binding as ib, image_rows_binding as irb, image_tiles_binding as itb, ops
    want = headers.header_prototypes(headers.include(HEADER))
    assert set(want) == set(irb._EXPORTS) == NAMES
    for name, args in want.items():
        assert len(irb._EXPORTS[name]) == len(args) == 21, name
        for i, (got, exp) in enumerate(zip(irb._EXPORTS[name], args)):
            assert got == exp, "%s: argument %d is %s in the binding, %s in the header" % (name, i, got.__name__, exp.__name__)
        assert args[-1] == C.c_void_p                  # the stream comes last
    lib = irb.load()
    for name in want:
        assert hasattr(lib, name) and getattr(lib, name).argtypes == irb._EXPORTS[name] and getattr(lib, name).restype is C.c_int
    base = headers.header_names(headers.include("x2i.h"))
    assert len(base) == 80                             # x2i.h still has its 80 names
    assert not (base & NAMES) and not (set(_lib._EXPORTS) & NAMES) and not (set(ib._EXPORTS) & NAMES) and not (set(itb._EXPORTS) & NAMES)
    assert not any(hasattr(ops, n) for n in ("image_rows", "rows"))
    text = open(headers.include(HEADER)).read()
    assert '#include "../../../x2i.h"' in text and "Everything x2i_image.h says holds here" in text


def test_no_other_header_declares_the_name_and_the_new_directory_holds_one_header():
    others = [p for p in glob.glob(headers.include("**/*.h"), recursive=True) if os.path.realpath(p) != os.path.realpath(headers.include(HEADER))]
    assert len(others) == 18                           # x2i.h, the 16 closed ones and tiles/x2i_image_tiles.h
    for path in others:
        assert not (headers.header_names(path) & NAMES), path
    assert glob.glob(headers.include("frontend/rows/*.h")) == []
    assert sorted(os.listdir(headers.include("frontend/rows"))) == ["qwen"]
    assert sorted(os.listdir(headers.include("frontend/rows/qwen"))) == ["x2i_image_rows.h"]
    assert os.path.exists(os.path.join(headers.ROOT, "x2i_amd", "image_rows_binding.py"))
    assert not os.path.exists(os.path.join(headers.ROOT, "x2i_amd", "image_rows_ops.py"))
    assert len(glob.glob(os.path.join(headers.ROOT, "x2i_amd", "*_ops.py"))) == 13


def test_integration_md_names_the_header_and_the_entry_point():
    md = open(os.path.join(headers.ROOT, "INTEGRATION.md")).read()
    assert "Extension header `include/frontend/rows/qwen/x2i_image_rows.h`" in md
    assert all("`%s`" % n in md for n in NAMES)


def test_the_build_tracks_headers_under_include_frontend_rows_qwen(monkeypatch):
    from x2i_amd import build
    path = os.path.realpath(headers.include(HEADER))
    seen = []
    real = os.path.getmtime
    monkeypatch.setattr(build.os.path, "getmtime", lambda p: seen.append(os.path.realpath(p)) or real(p))
    build._newest_header()
    assert path in seen and os.path.realpath(os.path.join(build.CSRC, "image_passes.h")) in seen
    assert os.path.exists(os.path.join(build.CSRC, "image_rows.hip"))


def test_a_stale_library_is_reported_with_the_headers_path(monkeypatch):
    from x2i_amd import _lib, image_rows_binding as irb

    class Stale:
        pass

    monkeypatch.setattr(_lib, "load", lambda: Stale)
    with pytest.raises(_lib.X2IError, match=r"does not export x2i_image_rows \(include/frontend/rows/qwen/x2i_image_rows.h\)"):
        _lib.extension(HEADER, irb._EXPORTS)()


ORDER = ("frames", "fp", "rp", "n", "t", "iw", "ih", "ow", "oh", "hb", "hc", "hk", "vb", "vc", "vk", "lut", "out", "ois", "ors", "bf16", "st")


def _call(lib, **kw):
    """x2i_image_rows on never-dereferenced pointers: two clips of three 1280 x 720 frames -> 1484 x 812 (106 x 58 patches, two steps),
    rows 1216 apart, unless kw says otherwise"""
    fake = C.c_void_p(0x1000)
    d = dict(frames=fake, fp=3 * 1280 * 720, rp=3 * 1280, n=2, t=3, iw=1280, ih=720, ow=1484, oh=812, hb=fake, hc=fake, hk=5, vb=fake, vc=fake,
             vk=5, lut=fake, out=fake, ois=2 * 106 * 58 * 1216 + 7, ors=1216, bf16=0, st=None)
    d.update(kw)
    return lib.x2i_image_rows(*[d[k] for k in ORDER])


def test_the_entry_point_validates_its_arguments_without_a_gpu():
    from x2i_amd import image_binding as ib, image_rows_binding as irb
    lib = irb.load()
    err = lambda: lib.x2i_last_error()      # noqa: E731
    call = lambda **kw: _call(lib, **kw)    # noqa: E731
    assert ib.ksize(1280, 1484) == 5 and ib.ksize(720, 812) == 5
    # a valid call but for a misaligned `out` (the last check): everything before the launch passes
    assert call(out=C.c_void_p(0x1002)) == -3 and b"element size" in err()
    for k in ("frames", "lut", "out"):
        assert call(**{k: None}) == -1 and b"null" in err()
    assert call(n=0) == -2 and b"n_items=0" in err() and call(t=0) == -2 and b"t_in=0" in err() and call(n=-1, t=-1) == -2
    assert call(n=21845, t=3, out=C.c_void_p(0x1002)) == -3 and call(n=21846, t=3) == -2 and b"1..65535" in err()       # 65535 frames, 65538
    assert call(n=65536, t=65536) == -2 and call(n=65535, t=1, out=C.c_void_p(0x1002)) == -3 and call(n=65536, t=1) == -2
    assert call(iw=0) == -2 and b"in_w=0" in err() and call(ih=65536) == -2 and b"in_h=65536" in err()
    for ow in (1470, 1483, 0, 14, 11788):
        assert call(ow=ow) == -2 and b"out_w=%d must be a multiple of 28 in 28..11760" % ow in err()
    for oh in (798, 811, 0, 14, 11788):
        assert call(oh=oh) == -2 and b"out_h=%d must be a multiple of 28" % oh in err()
    assert call(rp=3 * 1280 - 1) == -2 and b"row_pitch=3839" in err() and call(fp=3 * 1280 * 720 - 1) == -2 and b"frame_pitch" in err()
    assert call(hk=7) == -2 and b"hk=7" in err() and b"ksize 5" in err() and call(vk=0) == -2 and b"vk=0" in err()
    assert call(hb=None) == -1 and b"hbound" in err() and call(hc=None) == -1 and call(vb=None) == -1 and b"vbound" in err() and call(vc=None) == -1
    # an axis that does not resize takes no tables: 1484 wide in, and 812 high in
    same = dict(iw=1484, rp=3 * 1484, fp=3 * 1484 * 720)
    assert call(hk=5, **same) == -2 and b"ksize 0" in err() and call(hk=0, **same) == -1 and b"exactly where in_w != out_w" in err()
    assert call(hk=0, hb=None, hc=None, out=C.c_void_p(0x1002), **same) == -3
    assert call(ih=812, fp=3 * 1280 * 812, vk=0) == -1 and b"exactly where in_h != out_h" in err()
    # the strides: a row holds 1176 values, an item grid_t * gh * gw = 2 * 58 * 106 rows
    rows = 2 * 58 * 106
    assert call(ors=1175) == -2 and b"out_row_stride=1175" in err() and call(ors=0) == -2 and call(ors=-1216) == -2
    assert call(ois=rows * 1216 - 1) == -2 and b"out_item_stride" in err() and call(ois=rows * 1216, out=C.c_void_p(0x1002)) == -3
    assert call(ors=1176, ois=rows * 1176, out=C.c_void_p(0x1002)) == -3 and call(ors=1176, ois=rows * 1176 - 1) == -2          # the tight strides
    assert call(t=4, out=C.c_void_p(0x1002)) == -3 and call(t=5) == -2           # two steps still, then three
    assert call(ors=1 << 62, ois=(1 << 63) - 1) == -2                            # no product that could wrap
    for k in ("hb", "hc", "vb", "vc", "lut"):
        assert call(**{k: C.c_void_p(0x1002)}) == -3 and b"4-byte aligned" in err()
    assert call(out=C.c_void_p(0x1001), bf16=1) == -3 and call(out=C.c_void_p(0x1002), bf16=1, n=0) == -2
    # the LDS plan is x2i_image.h's: refused exactly where image_binding.lds_plan refuses, before the alignment is looked at
    seen = set()
    for ih in (1489, 2990, 3000, 30000):
        try:
            fits = ib.lds_plan(ih, 28)[0] * 44 <= ib.LDS_BYTES
        except ib.X2IError:
            fits = False
        seen.add(fits)
        rc = call(ih=ih, oh=28, vk=ib.ksize(ih, 28), fp=3 * 1280 * ih, out=C.c_void_p(0x1002))
        assert (rc, b"LDS plan does not fit" in err()) == ((-3, False) if fits else (-2, True)), (ih, rc, err())
        if fits:
            assert irb.check_sizes(1280, ih, 1484, 28) == (1, 2, 106)
        else:
            with pytest.raises(ib.X2IError, match="LDS plan does not fit"):
                irb.check_sizes(1280, ih, 1484, 28)
    assert seen == {True, False}


def test_the_binding_refuses_what_the_launcher_refuses(monkeypatch):
    from x2i_amd import image_binding as ib, image_rows_binding as irb, ops
    assert irb.check_sizes(128, 128, 140, 140) == (1, 10, 10) and irb.check_sizes(37, 61, 28, 56, 1, 3) == (2, 4, 2)
    assert irb.check_sizes(4000, 300, 11760, 28, 5, 4) == (2, 2, 840)
    for args, msg in (((0, 480, 644, 476), "in_w=0"), ((640, 480, 630, 476), "out_w=630"), ((640, 480, 644, 11788), "out_h=11788"),
                      ((640, 480, 14, 28), "out_w=14"), ((640, 480, 644, 476, 0, 1), "n_items=0"), ((640, 480, 644, 476, 1, 0), "t_in=0"),
                      ((640, 480, 644, 476, 256, 256), "n_items=256 and t_in=256")):
        with pytest.raises(ib.X2IError, match=msg):
            irb.check_sizes(*args)
    # the buffer checks of the tensor wrapper, on CPU tensors: the device check is taken out, no pointer is used
    monkeypatch.setattr(ops, "_req", lambda t, dtype, name: None)
    frames, lut = torch.zeros(2 * 3 * 3 * 20 * 10, dtype=torch.uint8), torch.zeros(3, 256)
    hb, hc = torch.zeros(56, 2, dtype=torch.int32), torch.zeros(56, ib.ksize(20, 56), dtype=torch.int32)
    vb, vc = torch.zeros(28, 2, dtype=torch.int32), torch.zeros(28, ib.ksize(10, 28), dtype=torch.int32)
    rows = 2 * 2 * 4                                   # three frames: two steps of 2 x 4 patches
    ok = dict(frames=frames, in_w=20, in_h=10, row_pitch=60, frame_pitch=600, n_items=2, t_in=3, out_w=56, out_h=28, hbound=hb, hcoef=hc,
              vbound=vb, vcoef=vc, lut=lut, out=torch.zeros(rows * 1216 + 5 + (rows - 1) * 1216 + 1176), out_item_stride=rows * 1216 + 5,
              out_row_stride=1216)
    args = irb._rows_args(**ok)
    assert len(args) == 20 and args[3:9] == (2, 3, 20, 10, 56, 28) and args[-3:] == (rows * 1216 + 5, 1216, 0)
    assert irb._rows_args(**dict(ok, out=ok["out"].bfloat16()))[-1] == 1
    for change, msg in ((dict(out=ok["out"][:-1]), "do not fit"), (dict(out_item_stride=rows * 1216 - 1), "do not fit"),
                        (dict(out_row_stride=1175), "do not fit"), (dict(frames=frames[:-1]), "frames holds"), (dict(row_pitch=59), "frames holds"),
                        (dict(out=torch.zeros(40000, dtype=torch.float16)), "float32 or bfloat16"), (dict(t_in=4), "frames holds"),
                        (dict(hbound=None), "horizontal tables are missing"), (dict(vcoef=vc[:, :-1]), "vertical tables must be contiguous"),
                        (dict(in_h=28, frame_pitch=28 * 60, frames=torch.zeros(6 * 28 * 60, dtype=torch.uint8)), "vertical tables must be None"),
                        (dict(lut=torch.zeros(3, 255)), "lut must be")):
        with pytest.raises(ib.X2IError, match=msg):
            irb._rows_args(**dict(ok, **change))
