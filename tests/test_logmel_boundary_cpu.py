"""The extension header include/ext/x2i_logmel.h against its binding x2i_amd/logmel_binding.py, the built library, include/x2i.h, the
thirteen include/x2i_*.h headers and INTEGRATION.md (no GPU): what tests/test_extension_boundary_cpu.py does for those thirteen.  Also the
entry points' argument checks, which need no GPU, and the build's dependency on headers under include/ext/."""
import ctypes as C
import glob
import os

from tests import headers

HEADER = "ext/x2i_logmel.h"
NAMES = {"x2i_logmel_spectrum_f32", "x2i_logmel_finish"}      # written out, so that a renamed export fails


def test_header_matches_its_binding_and_the_library_exports_it():
    from x2i_amd import _lib, logmel_binding as lb, ops
    want = headers.header_prototypes(headers.include(HEADER))
    assert set(want) == set(lb._EXPORTS) == NAMES
    for name, args in want.items():
        assert len(lb._EXPORTS[name]) == len(args), name
        for i, (got, exp) in enumerate(zip(lb._EXPORTS[name], args)):
            assert got == exp, "%s: argument %d is %s in the binding, %s in the header" % (name, i, got.__name__, exp.__name__)
        assert args[-1] == C.c_void_p                  # the stream comes last
    lib = lb.load()
    for name in want:
        assert hasattr(lib, name) and getattr(lib, name).argtypes == lb._EXPORTS[name] and getattr(lib, name).restype is C.c_int
    base = headers.header_names(headers.include("x2i.h"))
    assert len(base) == 80 and not (base & NAMES) and not (set(_lib._EXPORTS) & NAMES)
    assert not any(hasattr(ops, n) for n in ("logmel_spectrum", "logmel_finish", "spectrum", "finish"))
    text = open(headers.include(HEADER)).read()
    assert '#include "../x2i.h"' in text


def test_no_other_header_declares_these_names_and_the_closed_sets_are_as_they_were():
    others = sorted(glob.glob(headers.include("x2i_*.h")))
    assert len(others) == 13
    for path in others:
        assert not (headers.header_names(path) & NAMES), path
    assert sorted(os.path.basename(p) for p in glob.glob(headers.include("ext/*.h"))) == ["x2i_logmel.h"]
    assert not os.path.exists(os.path.join(headers.ROOT, "x2i_amd", "logmel_ops.py"))


def test_integration_md_names_the_header_and_both_entry_points():
    md = open(os.path.join(headers.ROOT, "INTEGRATION.md")).read()
    assert "Extension header `include/ext/x2i_logmel.h`" in md
    assert all("`%s`" % n in md for n in NAMES)


def test_the_build_tracks_headers_under_include_ext(monkeypatch):
    from x2i_amd import build
    path = os.path.realpath(headers.include(HEADER))
    seen = []
    real = os.path.getmtime
    monkeypatch.setattr(build.os.path, "getmtime", lambda p: seen.append(os.path.realpath(p)) or real(p))
    build._newest_header()
    assert path in seen


def test_a_stale_library_is_reported_with_the_headers_path(monkeypatch):
    import pytest

    from x2i_amd import _lib, logmel_binding as lb

    class Stale:
        pass

    monkeypatch.setattr(_lib, "load", lambda: Stale)
    with pytest.raises(_lib.X2IError, match=r"does not export x2i_logmel_\w+ \(include/ext/x2i_logmel.h\)"):
        _lib.extension(HEADER, lb._EXPORTS)()


def test_entry_points_validate_their_arguments_without_a_gpu():
    from x2i_amd import logmel_binding as lb
    lib = lb.load()
    fake = C.c_void_p(0x1000)  # never dereferenced: validation fails first
    err = lambda: lib.x2i_last_error()
    B, N, M = 2, 480000, 80
    lgf, pf = lb.workspace_floats(B, N, M)
    assert (lgf, pf) == (2 * 80 * 3000, 2 * 94)
    spec = lambda **kw: lib.x2i_logmel_spectrum_f32(*[kw.get(k, d) for k, d in (
        ("wave", fake), ("ldw", N), ("n", fake), ("dft", fake), ("fbank", fake), ("lg", fake), ("lgf", lgf), ("part", fake), ("pf", pf), ("B", B),
        ("N", N), ("M", M), ("st", None))])
    fin = lambda **kw: lib.x2i_logmel_finish(*[kw.get(k, d) for k, d in (
        ("lg", fake), ("lgf", lgf), ("part", fake), ("pf", pf), ("n", fake), ("out", fake), ("obs", M * 3000), ("old", 3000), ("B", B), ("N", N),
        ("M", M), ("T_out", 3000), ("bf16", 0), ("st", None))])
    for f in (spec, fin):
        assert f(B=0) == -2 and b"B=0" in err() and f(B=65536) == -2 and b"B=65536" in err()
        assert f(N=480001) == -2 and b"N_max=480001" in err() and f(N=160) == -2 and b"N_max=160" in err() and f(N=0) == -2
        assert f(M=0) == -2 and b"n_mels=0" in err() and f(M=129) == -2 and b"n_mels=129" in err()
        assert f(lgf=lgf - 1) == -1 and b"lg_floats" in err() and f(pf=pf - 1) == -1 and b"part_floats" in err()
        assert f(lg=C.c_void_p(0x1002)) == -3 and b"aligned" in err() and f(part=C.c_void_p(0x1001)) == -3 and f(n=C.c_void_p(0x1002)) == -3
        for k in ("lg", "part", "n"):
            assert f(**{k: None}) == -1 and b"null" in err()
    assert spec(ldw=0) == -2 and b"ldw=0" in err()
    assert spec(wave=C.c_void_p(0x1002)) == -3 and spec(dft=C.c_void_p(0x1004)) == -3 and spec(fbank=C.c_void_p(0x1008)) == -3 and b"16-byte" in err()
    for k in ("wave", "dft", "fbank"):
        assert spec(**{k: None}) == -1 and b"null" in err()
    assert fin(T_out=0) == -2 and b"T_out=0" in err()
    assert fin(old=2999) == -2 and b"out_ld=2999" in err() and fin(obs=M * 3000 - 1) == -2 and b"out_batch_stride" in err()
    assert fin(out=C.c_void_p(0x1002)) == -3 and fin(out=C.c_void_p(0x1002), bf16=1, T_out=0) == -2
    assert fin(out=C.c_void_p(0x1001), bf16=1) == -3 and b"element size" in err()
    assert fin(out=None) == -1 and b"null" in err()
