"""Every extension header include/x2i_<name>.h against its binding x2i_amd/<name>_ops.py, the built library, include/x2i.h, every other
extension header and INTEGRATION.md (no GPU).  What belongs to one header alone (its constants, its text) is tested beside that port."""
import ctypes as C
import glob
import importlib
import itertools
import os

import pytest

from tests import headers

ROOT = headers.ROOT
HEADERS = sorted(os.path.basename(p) for p in glob.glob(headers.include("x2i_*.h")))

# written out, so that a renamed export fails even where header and binding were renamed together
NAMES = {
    "x2i_t5.h": {"x2i_t5_attention_bf16", "x2i_t5_head_split_bf16", "x2i_t5_rms_rows_bf16", "x2i_t5_gated_gelu_bf16"},
    "x2i_clip.h": {"x2i_clip_attention_bf16", "x2i_clip_embed_bf16", "x2i_clip_quick_gelu_bf16", "x2i_clip_pool_bf16"},
    "x2i_qwen.h": {"x2i_qwen_attention_bf16", "x2i_qwen_rope_split_bf16", "x2i_qwen_swiglu_bf16"},
    "x2i_vit.h": {"x2i_vit_attention_bf16", "x2i_vit_rope_split_bf16"},
    "x2i_qwen_decode.h": {"x2i_qwen_decode_rope_append_bf16", "x2i_qwen_decode_attention_bf16", "x2i_qwen_decode_linear_bf16"},
    "x2i_qwen_head.h": {"x2i_qwen_head_logits_argmax_bf16", "x2i_qwen_head_select"},
    "x2i_merge.h": {"x2i_merge_rank_i32", "x2i_embed_merge_bf16"},
    "x2i_siglip.h": {"x2i_siglip_patch_rows_bf16", "x2i_siglip_add_positions_bf16", "x2i_siglip_head_split_bf16"},
    "x2i_resampler.h": {"x2i_resampler_attention_bf16", "x2i_resampler_ln_pos_bf16", "x2i_resampler_kv_split_bf16"},
    "x2i_whisper.h": {"x2i_whisper_mel_rows_bf16", "x2i_whisper_pool_rows_bf16"},
    "x2i_internvit.h": {"x2i_internvit_patch_rows_bf16", "x2i_internvit_embed_bf16", "x2i_internvit_shuffle_ln_bf16"},
    "x2i_qwen_decode_w8.h": {"x2i_qwen_decode_linear_w8_bf16"},
    "x2i_qwen_extend.h": {"x2i_qwen_extend_rope_split_bf16", "x2i_qwen_extend_attention_bf16"},
}
# wrappers of these names belong in the header's own module, never in ops
NOT_IN_OPS = {
    "x2i_vit.h": ("vit_attention", "vit_rope_split"),
    "x2i_siglip.h": ("siglip_patch_rows", "siglip_add_positions", "siglip_head_split"),
    "x2i_resampler.h": ("resampler_attention", "resampler_ln_pos", "resampler_kv_split"),
    "x2i_whisper.h": ("mel_rows", "pool_rows"),
    "x2i_internvit.h": ("internvit_patch_rows", "internvit_embed", "internvit_shuffle_ln"),
}
# INTEGRATION.md introduces every header as "Extension header `include/...`" but these two, which it names in backticks in a sentence
PLAIN_MENTION = {"x2i_t5.h", "x2i_qwen_decode_w8.h"}


def _module(header):
    return importlib.import_module("x2i_amd.%s_ops" % header[len("x2i_"):-len(".h")])


def test_every_header_has_a_binding_module_and_every_binding_module_a_header():
    modules = sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "x2i_amd", "*_ops.py")))
    assert modules == sorted(h[len("x2i_"):-len(".h")] + "_ops.py" for h in HEADERS)
    assert set(HEADERS) == set(NAMES) and len(HEADERS) == 13


@pytest.mark.parametrize("header", HEADERS)
def test_extension_header_matches_its_binding_and_the_library_exports_it(header):
    from x2i_amd import _lib, ops
    mod = _module(header)
    want = headers.header_prototypes(headers.include(header))
    assert set(want) == set(mod._EXPORTS) == NAMES[header]
    for name, args in want.items():
        assert len(mod._EXPORTS[name]) == len(args), name
        for i, (got, exp) in enumerate(zip(mod._EXPORTS[name], args)):
            assert got == exp, "%s: argument %d is %s in the binding, %s in the header" % (name, i, got.__name__, exp.__name__)
        assert args[-1] == C.c_void_p                  # the stream comes last
    lib = mod.load()
    for name in want:
        assert hasattr(lib, name) and getattr(lib, name).argtypes == mod._EXPORTS[name]
    # the closed table of include/x2i.h is as it was, and no name of this header is in it
    base = headers.header_names(headers.include("x2i.h"))
    assert len(base) == 80 and not (base & set(want)) and not (set(_lib._EXPORTS) & set(want))
    assert not any(hasattr(ops, n) for n in NOT_IN_OPS.get(header, ()))
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert ("`include/%s`" if header in PLAIN_MENTION else "Extension header `include/%s`") % header in md
    assert all("`%s`" % n in md for n in want)


def test_no_two_extension_headers_declare_the_same_name():
    names = {h: headers.header_names(headers.include(h)) for h in HEADERS}
    for a, b in itertools.combinations(HEADERS, 2):
        assert not (names[a] & names[b]), "%s and %s both declare %s" % (a, b, sorted(names[a] & names[b]))


def test_a_library_without_a_headers_symbol_is_reported_as_a_stale_build(monkeypatch):
    from x2i_amd import _lib

    class Stale:
        x2i_here = type("Fn", (), {})()

    monkeypatch.setattr(_lib, "load", lambda: Stale)
    load = _lib.extension("x2i_none.h", {"x2i_here": [C.c_void_p], "x2i_gone": [C.c_void_p]})
    with pytest.raises(_lib.X2IError) as e:
        load()
    msg = str(e.value)
    assert _lib.LIB_PATH in msg and "does not export x2i_gone" in msg and "(include/x2i_none.h)" in msg
    assert "stale build? run `python -m x2i_amd.build`" in msg
    assert Stale.x2i_here.argtypes == [C.c_void_p] and Stale.x2i_here.restype is C.c_int      # bound up to the missing one
    Stale.x2i_gone = type("Fn", (), {})()
    assert load() is Stale and Stale.x2i_gone.argtypes == [C.c_void_p]                       # a failed bind is not remembered as done
