"""Reading the prototypes of the C headers under include/ (a helper of the boundary tests; it holds no tests)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {"int32_t": C.c_int32, "int": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "x2i_stream_t": C.c_void_p}


def include(name):
    return os.path.join(ROOT, "include", name)


def raw_prototypes(text):
    """[(return type, name, parameter text)] of every `<type> x2i_...(...);` of a header's text, comments removed"""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.findall(r"^(int|int64_t|const char\*)\s+(x2i_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M)


def header_names(path):
    return {name for _, name, _ in raw_prototypes(open(path).read())}


def header_prototypes(path):
    """{export: [ctypes argument types]} of an extension header: every prototype returns int, a pointer of any kind is device memory
    (tests/test_boundary_cpu.py reads include/x2i.h, whose prototypes also take structs and return other types)"""
    out = {}
    for ret, name, params in raw_prototypes(open(path).read()):
        assert ret == "int", name
        args = []
        for p in " ".join(params.split()).split(","):
            words = [w for w in p.replace("*", " * ").split() if w != "const"]
            assert len(words) >= 2, p                  # a type and a name
            words = words[:-1] if words[-1] != "*" else words
            args.append(C.c_void_p if "*" in words else SCALARS[words[0]])
        out[name] = args
    return out
