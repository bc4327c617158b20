"""The extension header include/ext/sample/x2i_sample.h against its binding x2i_amd/sample_binding.py, the built library, include/x2i.h, the
closed sets of headers and INTEGRATION.md (no GPU): what tests/test_logmel_boundary_cpu.py does for the log-mel header.  Also the entry point's
argument checks, which need no GPU, and the build's dependency on headers in subdirectories of include/ext/."""
import ctypes as C
import glob
import os

from tests import headers

HEADER = "ext/sample/x2i_sample.h"
NAMES = {"x2i_sample_select_f32"}      # written out, so that a renamed export fails


def test_header_matches_its_binding_and_the_library_exports_it():
    from x2i_amd import _lib, ops, sample_binding as sb
    want = headers.header_prototypes(headers.include(HEADER))
    assert set(want) == set(sb._EXPORTS) == NAMES
    for name, args in want.items():
        assert len(sb._EXPORTS[name]) == len(args), name
        for i, (got, exp) in enumerate(zip(sb._EXPORTS[name], args)):
            assert got == exp, "%s: argument %d is %s in the binding, %s in the header" % (name, i, got.__name__, exp.__name__)
        assert args[-1] == C.c_void_p                  # the stream comes last
    lib = sb.load()
    for name in want:
        assert hasattr(lib, name) and getattr(lib, name).argtypes == sb._EXPORTS[name] and getattr(lib, name).restype is C.c_int
    base = headers.header_names(headers.include("x2i.h"))
    assert len(base) == 80 and not (base & NAMES) and not (set(_lib._EXPORTS) & NAMES)
    assert not any(hasattr(ops, n) for n in ("sample_select", "sample", "select_sampled"))        # no wrapper of it in ops
    text = open(headers.include(HEADER)).read()
    assert '#include "../../x2i.h"' in text
    # the macros the binding restates
    assert "#define X2I_SAMPLE_DIAG_FLOATS %d\n" % sb.DIAG_FLOATS in text and "#define X2I_SAMPLE_MASS_BITS %d\n" % sb.MASS_BITS in text
    assert "#define X2I_SAMPLE_HEAD_WS_FLOATS(B, V) (4 + 2 * (int64_t)(B) * (((int64_t)(V) + 15) / 16))" in text
    from x2i_amd import qwen_head_ops
    for B, V in ((1, 1), (3, 17), (8, 151936)):
        assert sb.head_workspace_floats(B, V) == qwen_head_ops.workspace_floats(B, V)
    from tests import sample_ref
    assert sample_ref.MASS_BITS == sb.MASS_BITS


def test_no_other_header_declares_the_name_and_the_closed_sets_are_as_they_were():
    others = sorted(glob.glob(headers.include("x2i_*.h")))
    assert len(others) == 13
    for path in others + [headers.include("ext/x2i_logmel.h")]:
        assert not (headers.header_names(path) & NAMES), path
    assert sorted(os.path.basename(p) for p in glob.glob(headers.include("ext/*.h"))) == ["x2i_logmel.h"]
    assert sorted(os.path.relpath(p, headers.include("ext")) for p in glob.glob(headers.include("ext/*/*.h"))) == ["sample/x2i_sample.h"]
    assert len(glob.glob(os.path.join(headers.ROOT, "x2i_amd", "*_ops.py"))) == 13
    assert not os.path.exists(os.path.join(headers.ROOT, "x2i_amd", "sample_ops.py"))


def test_integration_md_names_the_header_and_the_entry_point():
    md = open(os.path.join(headers.ROOT, "INTEGRATION.md")).read()
    assert "Extension header `include/ext/sample/x2i_sample.h`" in md
    assert all("`%s`" % n in md for n in NAMES)


def test_the_build_tracks_headers_in_subdirectories_of_include_ext(monkeypatch):
    from x2i_amd import build
    paths = [os.path.realpath(headers.include(h)) for h in (HEADER, "ext/x2i_logmel.h", "x2i.h")]
    seen = []
    real = os.path.getmtime
    monkeypatch.setattr(build.os.path, "getmtime", lambda p: seen.append(os.path.realpath(p)) or real(p))
    build._newest_header()
    assert all(p in seen for p in paths)


def test_a_stale_library_is_reported_with_the_headers_path(monkeypatch):
    import pytest

    from x2i_amd import _lib, sample_binding as sb

    class Stale:
        pass

    monkeypatch.setattr(_lib, "load", lambda: Stale)
    with pytest.raises(_lib.X2IError, match=r"does not export x2i_sample_select_f32 \(include/ext/sample/x2i_sample.h\)"):
        _lib.extension(HEADER, sb._EXPORTS)()


def test_the_entry_point_validates_its_arguments_without_a_gpu():
    from x2i_amd import sample_binding as sb
    lib = sb.load()
    fake = C.c_void_p(0x1000)  # never dereferenced: validation fails first
    err = lambda: lib.x2i_last_error()
    B, V = 2, 1000
    wsf = sb.head_workspace_floats(B, V)
    f = lambda **kw: lib.x2i_sample_select_f32(*[kw.get(k, d) for k, d in (
        ("logits", fake), ("ldl", V), ("ws", fake), ("wsf", wsf), ("T", 0.7), ("top_k", 50), ("top_p", 0.8), ("rng", fake), ("u_in", None),
        ("diag", None), ("step", fake), ("token", fake), ("seq", fake), ("ld_seq", 16), ("ncols", 16), ("lengths", fake), ("done", fake),
        ("eos", fake), ("n_eos", 2), ("pad", 0), ("seen", fake), ("ld_seen", V), ("B", B), ("V", V), ("st", None))])
    for k in ("logits", "ws", "step", "token", "seq", "lengths", "done"):
        assert f(**{k: None}) == -1 and b"null" in err(), k
    assert f(rng=None) == -1 and b"rng and u_in" in err() and f(eos=None) == -1 and b"eos" in err()
    assert f(B=0) == -2 and b"B=0" in err() and f(B=9) == -2 and b"B=9" in err()
    assert f(V=0) == -2 and b"V=0" in err() and f(V=-5) == -2 and f(V=2 ** 29 + 1, ldl=2 ** 30, ld_seen=2 ** 30, wsf=2 ** 40) == -2
    for T in (0.0, -1.0, float("inf"), float("nan")):
        assert f(T=T) == -1 and b"temperature" in err(), T
    assert f(top_k=-1) == -1 and b"top_k=-1" in err()
    for p in (0.0, -0.5, 1.0000001, float("nan")):
        assert f(top_p=p) == -1 and b"top_p" in err(), p
    assert f(n_eos=-1) == -1 and f(n_eos=9) == -1 and b"n_eos=9" in err()
    assert f(pad=-1) == -1 and f(pad=V) == -1 and b"pad=1000" in err()
    assert f(ldl=V - 1) == -2 and b"ldl" in err() and f(ncols=-1) == -2 and f(ld_seq=15) == -2 and f(ld_seen=V - 1) == -2
    assert f(wsf=wsf - 1) == -2 and b"workspace too small" in err()
    odd = lambda a: C.c_void_p(0x1000 + a)
    for k, a in (("ws", 8), ("rng", 4), ("token", 4), ("seq", 4), ("lengths", 4), ("eos", 4), ("logits", 2), ("u_in", 2), ("diag", 2), ("step", 2)):
        assert f(**{k: odd(a)}) == -3 and b"aligned" in err(), k
    # the largest values pass the checks that come before the workspace's size
    assert f(top_k=2 ** 31 - 1, top_p=1.0, T=1e-30, wsf=0) == -2 and b"workspace too small" in err()
    # (a call that passes every check launches, which needs a GPU: tests/test_sample_gpu.py)
