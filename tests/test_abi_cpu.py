"""CPU tests of the binding's one source: the reader of include/fsg_hip.h (fissure_segmentation_amd/_abi.py) on header text written
here, the struct layouts and constants it derives against what the C compiler makes of the real header, and the library's dynamic
symbols against the header's declarations, both ways."""
import ctypes
import os
import shutil
import subprocess

import pytest

from fissure_segmentation_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float

SYNTHETIC = """
/* a comment with a ( and a ; and a call fsg_foo( that declares nothing;
 * int fsg_in_comment(int a);
 */
#ifndef FSG_SYNTHETIC_H
#define FSG_SYNTHETIC_H
#define FSG_OK 0
#define FSG_BASE 0x10          /* hex; this comment has a ( too */
#define FSG_MAX_JOBS (1 << 3)
#define FSG_FLAGS ((1 << 11) | FSG_BASE | 3u)   // derived from an earlier define
#define FSG_SIGMA 255.0f
typedef void *fsg_stream_t;
typedef struct fsg_jobs {
    const float *src[FSG_MAX_JOBS], *dst[FSG_MAX_JOBS];   /* two declarators, one line */
    int64_t ld[FSG_MAX_JOBS];
    int32_t rows[4], n;
    const float *a, *b;
    float slope;
} fsg_jobs;
int fsg_version(void);
const char *fsg_last_error(void);
size_t fsg_bytes(long M, size_t have, int C);
int fsg_run(const float *x, int64_t stride,   // fsg_not_this_one(int a);
            const fsg_jobs *jobs, double tol,
            float slope, int32_t *out, fsg_stream_t stream);
#endif
"""


def test_parser_on_synthetic_header():
    defines, structs, sigs = _abi.parse(SYNTHETIC)
    assert defines == {"FSG_OK": 0, "FSG_BASE": 16, "FSG_MAX_JOBS": 8, "FSG_FLAGS": 2048 | 16 | 3, "FSG_SIGMA": 255.0}
    assert type(defines["FSG_SIGMA"]) is float and type(defines["FSG_FLAGS"]) is int
    assert set(sigs) == {"fsg_version", "fsg_last_error", "fsg_bytes", "fsg_run"}   # nothing out of a comment
    assert sigs["fsg_version"] == ([], I)                                            # (void)
    assert sigs["fsg_last_error"] == ([], ctypes.c_char_p)
    assert sigs["fsg_bytes"] == ([ctypes.c_long, ctypes.c_size_t, I], ctypes.c_size_t)
    assert sigs["fsg_run"] == ([P, L, P, ctypes.c_double, F, P, P], I)               # three lines; pointer to struct; handle
    jobs = structs["fsg_jobs"]
    assert list(structs) == ["fsg_jobs"] and issubclass(jobs, ctypes.Structure)
    assert [(n, t) for n, t in jobs._fields_] == [("src", P * 8), ("dst", P * 8), ("ld", L * 8), ("rows", ctypes.c_int32 * 4),
                                                  ("n", ctypes.c_int32), ("a", P), ("b", P), ("slope", F)]
    assert jobs.slope.offset == 3 * 64 + 16 + 4 + 4 + 16 and ctypes.sizeof(jobs) == jobs.slope.offset + 8   # trailing scalar, padded


@pytest.mark.parametrize("text, offender", [
    ("int fsg_f(unsigned n);", "unsigned"),                                         # a type the table does not know
    ("int fsg_f(int a, wchar_t b);", "wchar_t"),
    ("short fsg_f(int a);", "short"),
    ("typedef struct fsg_s { int n; bool flag; } fsg_s;", "bool"),
    ("typedef struct fsg_s { float *p[FSG_UNDEFINED_MAX]; int n; } fsg_s;", "FSG_UNDEFINED_MAX"),
    ("#define FSG_A (FSG_LATER | 1)\n#define FSG_LATER 2", "FSG_A"),                 # only EARLIER defines may be named
    ("#define FSG_A sizeof(int)", "FSG_A"),
])
def test_parser_refuses_what_it_does_not_know(text, offender):
    with pytest.raises(ValueError, match=offender):
        _abi.parse(text)
    if text.startswith("int fsg_f("):
        with pytest.raises(ValueError, match="fsg_f"):                              # and names the function
            _abi.parse(text)


def test_missing_header_is_an_import_error():
    path = os.path.join(ROOT, "include", "no_such_header.h")
    with pytest.raises(ImportError, match="no_such_header.h"):
        _abi.load(path)


def test_binding_is_the_parsed_header():
    defines, structs, sigs = _abi.load(os.path.join(ROOT, "include", "fsg_hip.h"))
    assert _lib.HEADER_PATH and os.path.samefile(_lib.HEADER_PATH, os.path.join(ROOT, "include", "fsg_hip.h"))
    assert sigs == _lib.SIGNATURES and defines == _lib.DEFINES and list(structs) == list(_lib.STRUCTS)
    assert len(sigs) >= 182 and len(structs) >= 11
    for name, (args, res) in sigs.items():
        fn = getattr(_lib.lib, name)
        assert list(fn.argtypes) == args and fn.restype is res, name
    for name, value in defines.items():
        assert getattr(_lib, name[len("FSG_"):]) == value, name
    assert _lib.PWRowGemmArgs is _lib.STRUCTS["fsg_pw_rowgemm_args"] and _lib.AdamSegments is _lib.STRUCTS["fsg_adam_segments"]


def test_layouts_and_constants_match_the_c_compiler(tmp_path):
    """sizeof / offsetof of every struct and the value of every define, as the host C compiler sees the real header"""
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no host C compiler (cc / gcc): it is what builds oracle/, and this check needs it"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "fsg_hip.h"', "int main(void) {"]
    for name, cls in _lib.STRUCTS.items():
        lines.append(f'    printf("{name} sizeof %zu\\n", sizeof({name}));')
        lines += [f'    printf("{name} {f} %zu\\n", offsetof({name}, {f}));' for f, _ in cls._fields_]
    lines += [f'    printf("{k} define %lld\\n", (long long)({k}));' for k, v in _lib.DEFINES.items() if isinstance(v, int)]
    lines += [f'    printf("{k} define %.17g\\n", (double)({k}));' for k, v in _lib.DEFINES.items() if isinstance(v, float)]
    lines += ["    return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    seen = {tuple(ln.split()[:2]): float(ln.split()[2]) if set(ln.split()[2]) & set(".en") else int(ln.split()[2])
            for ln in out.splitlines()}
    want = {(k, "define"): v if isinstance(v, int) else ctypes.c_float(v).value for k, v in _lib.DEFINES.items()}   # `f` literals
    for name, cls in _lib.STRUCTS.items():
        want[(name, "sizeof")] = ctypes.sizeof(cls)
        want.update({(name, f): getattr(cls, f).offset for f, _ in cls._fields_})
    assert len(want) > 200 and seen == want, {k: (seen.get(k), want.get(k)) for k in set(seen) | set(want) if seen.get(k) != want.get(k)}
    assert seen[("FSG_ELASTIC_MAX_SIGMA", "define")] == 255.0 and seen[("FSG_KNN_DBG_BF16", "define")] == 1 << 30


# test / tool hooks the library exports but the public header deliberately does not declare
DEBUG_HOOKS = {"fsg_debug_ec2_use_fp32_mfma", "fsg_debug_knn_split_stats", "fsg_debug_knn_split_stamps", "fsg_debug_knn_refine_stamps"}


def test_exports_and_header_agree_both_ways():
    """every declared name is exported (the import already bound each one), and every `fsg_*` the library defines is declared --
    but for the fsg_debug_* hooks of tests and tools, which are deliberately not part of the public header"""
    nm = shutil.which("nm")
    assert nm, "no `nm` (binutils): this check needs it"
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("fsg_")}
    declared = set(_lib.SIGNATURES)
    assert declared - exported == set()
    assert exported - declared == DEBUG_HOOKS
    assert all(name.startswith("fsg_debug_") for name in DEBUG_HOOKS)
