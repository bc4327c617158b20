"""The extension header include/frontend/x2i_image.h against its binding x2i_amd/image_binding.py, the built library, include/x2i.h, the
other headers and INTEGRATION.md (no GPU): what tests/test_extension_boundary_cpu.py does for the thirteen include/x2i_*.h headers.  Also the
entry point's argument checks, which need no GPU, the binding's own copy of the LDS plan against the launcher's refusals, and the build's
dependency on headers under include/frontend/."""
import ctypes as C
import glob
import os

import pytest

from tests import headers

HEADER = "frontend/x2i_image.h"
NAMES = {"x2i_image_frontend"}      # written out, so that a renamed export fails


def test_header_matches_its_binding_and_the_library_exports_it():
    from x2i_amd import _lib, image_binding as ib, ops
    want = headers.header_prototypes(headers.include(HEADER))
    assert set(want) == set(ib._EXPORTS) == NAMES
    for name, args in want.items():
        assert len(ib._EXPORTS[name]) == len(args), name
        for i, (got, exp) in enumerate(zip(ib._EXPORTS[name], args)):
            assert got == exp, "%s: argument %d is %s in the binding, %s in the header" % (name, i, got.__name__, exp.__name__)
        assert args[-1] == C.c_void_p                  # the stream comes last
    lib = ib.load()
    for name in want:
        assert hasattr(lib, name) and getattr(lib, name).argtypes == ib._EXPORTS[name] and getattr(lib, name).restype is C.c_int
    base = headers.header_names(headers.include("x2i.h"))
    assert len(base) == 80 and not (base & NAMES) and not (set(_lib._EXPORTS) & NAMES)
    assert not any(hasattr(ops, n) for n in ("image_frontend", "frontend"))
    assert '#include "../x2i.h"' in open(headers.include(HEADER)).read()


def test_no_other_header_declares_the_name_and_the_closed_sets_are_as_they_were():
    others = sorted(glob.glob(headers.include("x2i_*.h")))
    assert len(others) == 13
    for path in others + glob.glob(headers.include("ext/*.h")) + glob.glob(headers.include("ext/*/*.h")):
        assert not (headers.header_names(path) & NAMES), path
    assert sorted(os.path.basename(p) for p in glob.glob(headers.include("ext/*.h"))) == ["x2i_logmel.h"]
    assert sorted(os.path.basename(p) for p in glob.glob(headers.include("ext/*/*.h"))) == ["x2i_sample.h"]
    assert sorted(os.path.basename(p) for p in glob.glob(headers.include("frontend/*.h"))) == ["x2i_image.h"]
    assert len(glob.glob(os.path.join(headers.ROOT, "x2i_amd", "*_ops.py"))) == 13
    assert not os.path.exists(os.path.join(headers.ROOT, "x2i_amd", "image_ops.py"))


def test_integration_md_names_the_header_and_the_entry_point():
    md = open(os.path.join(headers.ROOT, "INTEGRATION.md")).read()
    assert "Extension header `include/frontend/x2i_image.h`" in md
    assert all("`%s`" % n in md for n in NAMES)


def test_the_build_tracks_headers_under_include_frontend(monkeypatch):
    from x2i_amd import build
    path = os.path.realpath(headers.include(HEADER))
    seen = []
    real = os.path.getmtime
    monkeypatch.setattr(build.os.path, "getmtime", lambda p: seen.append(os.path.realpath(p)) or real(p))
    build._newest_header()
    assert path in seen


def test_a_stale_library_is_reported_with_the_headers_path(monkeypatch):
    from x2i_amd import _lib, image_binding as ib

    class Stale:
        pass

    monkeypatch.setattr(_lib, "load", lambda: Stale)
    with pytest.raises(_lib.X2IError, match=r"does not export x2i_image_frontend \(include/frontend/x2i_image.h\)"):
        _lib.extension(HEADER, ib._EXPORTS)()


ORDER = ("frames", "fp", "rp", "n", "iw", "ih", "ow", "oh", "hb", "hc", "hk", "vb", "vc", "vk", "lut", "out", "ofs", "ors", "bf16", "st")


def _call(lib, **kw):
    """x2i_image_frontend on never-dereferenced pointers: 1280 x 720 -> 602 x 336, two frames, unless kw says otherwise"""
    fake = C.c_void_p(0x1000)
    d = dict(frames=fake, fp=3 * 1280 * 720, rp=3 * 1280, n=2, iw=1280, ih=720, ow=602, oh=336, hb=fake, hc=fake, hk=11, vb=fake, vc=fake, vk=11,
             lut=fake, out=fake, ofs=42 * 14 * 1032, ors=14 * 1032, bf16=0, st=None)
    d.update(kw)
    return lib.x2i_image_frontend(*[d[k] for k in ORDER])


def test_the_entry_point_validates_its_arguments_without_a_gpu():
    from x2i_amd import image_binding as ib
    lib = ib.load()
    err = lambda: lib.x2i_last_error()      # noqa: E731
    call = lambda **kw: _call(lib, **kw)    # noqa: E731
    assert ib.ksize(1280, 602) == 11 and ib.ksize(720, 336) == 11 and ib.ksize(231, 28) == 35 and ib.ksize(120, 14) == 37 and ib.ksize(5, 5) == 0
    for k in ("frames", "lut", "out"):
        assert call(**{k: None}) == -1 and b"null" in err()
    assert call(n=0) == -2 and b"n=0" in err() and call(n=65536) == -2 and b"n=65536" in err()
    assert call(iw=0) == -2 and b"in_w=0" in err() and call(ih=65536) == -2 and b"in_h=65536" in err()
    assert call(ow=600) == -2 and b"out_w=600" in err() and call(ow=0) == -2 and call(ow=994) == -2 and b"out_w=994" in err()
    assert call(oh=335) == -2 and b"out_h=335" in err() and call(oh=0) == -2 and call(oh=994) == -2 and b"out_h=994" in err()
    assert call(rp=3 * 1280 - 1) == -2 and b"row_pitch=3839" in err() and call(fp=3 * 1280 * 720 - 1) == -2 and b"frame_pitch" in err()
    assert call(hk=13) == -2 and b"hk=13" in err() and b"ksize 11" in err() and call(vk=9) == -2 and b"vk=9" in err()
    assert call(hk=0) == -2 and call(vk=0) == -2
    assert call(hb=None) == -1 and b"hbound" in err() and call(hc=None) == -1 and call(vb=None) == -1 and b"vbound" in err() and call(vc=None) == -1
    # an axis that does not resize takes no tables
    same = dict(iw=602, rp=3 * 602, fp=3 * 602 * 720)
    assert call(hk=11, **same) == -2 and b"ksize 0" in err() and call(hk=0, **same) == -1 and b"exactly where in_w != out_w" in err()
    assert call(ih=336, vk=0) == -1 and b"exactly where in_h != out_h" in err()
    assert call(ors=14 * 1032 - 1) == -2 and b"out_row_stride" in err() and call(ofs=42 * 14 * 1032 - 1) == -2 and b"out_frame_stride" in err()
    for k in ("hb", "hc", "vb", "vc", "lut"):
        assert call(**{k: C.c_void_p(0x1002)}) == -3 and b"4-byte aligned" in err()
    assert call(out=C.c_void_p(0x1002)) == -3 and call(out=C.c_void_p(0x1001), bf16=1) == -3 and b"element size" in err()
    assert call(out=C.c_void_p(0x1002), bf16=1, n=0) == -2              # (an aligned bf16 pointer gets past the alignment check)


def test_the_lds_plan_of_the_binding_is_the_launchers():
    """rows * pitch must fit 64 KiB for one patch of columns at least: the launcher refuses exactly the scales lds_plan refuses, with a
    message, before any launch; a refused scale is what sends handoff.HipImage to the original processor"""
    from x2i_amd import image_binding as ib
    lib = ib.load()
    assert ib.lds_plan(720, 336) == (36, 4, 168) and ib.lds_plan(3000, 392) == (130, 4, 168) and ib.lds_plan(336, 336) == (14, 4, 168)
    # out_h = 14: the one patch row's taps reach every input row, so rows = in_h; 168, 84 and 44 bytes per row hold 390, 780 and 1489 rows
    want = {390: (390, 4, 168), 391: (391, 2, 84), 780: (780, 2, 84), 781: (781, 1, 44), 1489: (1489, 1, 44), 1490: None, 3000: None, 65535: None}
    for ih, plan in want.items():
        if plan is None:
            with pytest.raises(ib.X2IError, match="LDS plan does not fit"):
                ib.lds_plan(ih, 14)
        else:
            assert ib.lds_plan(ih, 14) == plan and plan[0] * plan[2] <= ib.LDS_BYTES
        # the launcher, with a misaligned `out` (checked after the plan) so that nothing is ever launched on these pointers
        rc = _call(lib, ih=ih, oh=14, vk=ib.ksize(ih, 14), fp=3 * 1280 * ih, ors=14 * 43, ofs=42 * 14 * 43, out=C.c_void_p(0x1002))
        msg = lib.x2i_last_error()
        assert (rc, b"LDS plan does not fit" in msg) == ((-2, True) if plan is None else (-3, False)), (ih, rc, msg)
