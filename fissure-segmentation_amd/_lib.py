"""ctypes binding of libfsg_hip.so (C ABI: include/fsg_hip.h).  No fallback: a missing library is an
ImportError, a failing call is a RuntimeError carrying fsg_last_error()."""
import ctypes
import os

import torch  # noqa: F401  -- must come first: brings torch's libamdhip64 into the process, which the
#                              library's DT_NEEDED libamdhip64.so.7 then resolves to (one HIP runtime)

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# (FSG_HIP_LIB: another BUILD of the same library -- tools/ use it to A/B compile-time variants on one box; still no fallback)
LIB_PATH = os.environ.get("FSG_HIP_LIB") or os.path.join(_HERE, "libfsg_hip.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      f"or `make -C {os.path.join(_HERE, 'csrc')}`; there is no CPU fallback.")

lib = ctypes.CDLL(LIB_PATH)

# Everything below comes from the header: SIGNATURES {entry point: ([argtypes], restype)}, STRUCTS {C name: ctypes.Structure} and
# DEFINES {"FSG_X": value}.  Nothing about an entry point, a struct layout or a limit is written in this file.
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "fsg_hip.h")
DEFINES, STRUCTS, SIGNATURES = _abi.load(HEADER_PATH)
for _name, (_args, _res) in SIGNATURES.items():
    _fn = getattr(lib, _name)  # AttributeError here = header and library out of sync
    _fn.argtypes, _fn.restype = _args, _res

globals().update((_k[len("FSG_"):], _v) for _k, _v in DEFINES.items())   # _lib.KNN_MAX_K = FSG_KNN_MAX_K, and so on for every define

PTLayerParams = STRUCTS["fsg_pt_layer_params"]
PTLayerGrads = STRUCTS["fsg_pt_layer_grads"]
GemmReduceJobs = STRUCTS["fsg_gemm_reduce_jobs"]
GemmSmallJobs = STRUCTS["fsg_gemm_small_jobs"]
AdamSegments = STRUCTS["fsg_adam_segments"]
EdgeWeightJobs = STRUCTS["fsg_edge_weight_jobs"]
EdgeWeightFoldJobs = STRUCTS["fsg_edge_weight_fold_jobs"]
PWRowGemmArgs = STRUCTS["fsg_pw_rowgemm_args"]
PWImageJobs = STRUCTS["fsg_pw_image_jobs"]
PWTnReduceJobs = STRUCTS["fsg_pw_tn_reduce_jobs"]
PWTnArgs = STRUCTS["fsg_pw_tn_args"]


_timing = None  # {entry point: [(start_event, end_event), ...]} while bench.py measures kernel durations


def start_timing():
    """Bracket every C-ABI call with HIP events on the stream it is launched on (torch's current stream)."""
    global _timing
    _timing = {}


def stop_timing():
    """-> {entry point: [milliseconds per call]} (synchronises)."""
    global _timing
    rec, _timing = _timing, None
    torch.cuda.synchronize()
    return {name: [s.elapsed_time(e) for s, e in evs] for name, evs in (rec or {}).items()}


_experiments = None


def experiments():
    """libfsg_hip_experiments.so: the superseded kNN designs (cross-checks for tests/, baselines for tools/) -- test
    infrastructure, loaded on first use, never by the product path"""
    global _experiments
    if _experiments is None:
        path = os.path.join(_HERE, "libfsg_hip_experiments.so")
        if not os.path.exists(path):
            raise ImportError(f"{path} not found: `make -C {os.path.join(_HERE, 'csrc')} all` builds it")
        x = ctypes.CDLL(path)
        x.fsg_knn_experiment_f32.argtypes, x.fsg_knn_experiment_f32.restype = SIGNATURES["fsg_knn_dense_f32"][0], ctypes.c_int
        x.fsg_last_error.restype = ctypes.c_char_p
        _experiments = x
    return _experiments


def workspace(entry, *dims, device):
    """the scratch that the `<entry>*` entry points ask for at these dims (`<entry>_workspace_bytes(*dims)`): a uint8 tensor of
    that many bytes (numel() is the byte count), or None -- a null pointer -- when the query returns 0"""
    nbytes = getattr(lib, entry + "_workspace_bytes")(*dims)
    return torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None


def call(name, *args):
    if _timing is None:
        rc = getattr(lib, name)(*args)
    else:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        rc = getattr(lib, name)(*args)
        e.record()
        _timing.setdefault(name, []).append((s, e))
    if rc != 0:
        raise RuntimeError(f"{name} failed (code {rc}): {lib.fsg_last_error().decode()}")
