"""Generate tests/golden/hessian_enhance.npz by running the REAL reference's Hessian enhancement filter on seeded inputs.

Runs only where the reference is checked out (oracle/make_golden.py: import_reference), on the CPU:
`data_processing.fissure_enhancement.HessianEnhancementFilter` with return_intermediate=True (which calls `fissure_filter`).
That module imports a long chain at its top (SimpleITK, skimage, sklearn, welford, pyamg, the dataset scripts ...) that the
filter never touches: a fallback on sys.meta_path answers any import that fails and was requested from a reference module
with an inert stand-in.  The inputs are regenerated from seeds (tests/hessian_oracle.py), only outputs are stored; no
reference source text is written.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_hessian.py
"""
import importlib.abc
import importlib.machinery
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]


def main():
    sys.dont_write_bytecode = True
    from oracle.make_golden import REF, _Inert, import_reference
    import numpy as np
    import torch
    import hessian_oracle as ho
    from golden_util import GOLDEN_DIR

    class Fallback(importlib.abc.MetaPathFinder, importlib.abc.Loader):
        """last on sys.meta_path: reached only when no real module exists"""

        def find_spec(self, name, path=None, target=None):
            f = sys._getframe(1)
            while f is not None and "importlib" in f.f_code.co_filename:
                f = f.f_back
            if f is None or not os.path.abspath(f.f_code.co_filename).startswith(REF + os.sep):
                return None
            return importlib.machinery.ModuleSpec(name, self, is_package=True)

        def create_module(self, spec):
            m = _Inert(spec.name)
            m.__path__ = []
            return m

        def exec_module(self, module):
            print("  stand-in for", module.__name__)

    import_reference()
    sys.meta_path.append(Fallback())
    from data_processing.fissure_enhancement import HessianEnhancementFilter

    torch.set_num_threads(8)
    out = dict(mu=ho.MU, sigma_hu=ho.SIGMA_HU)
    filt = HessianEnhancementFilter(ho.MU, ho.SIGMA_HU)
    for key, block in (("plain", None), ("block", ho.BLOCK_VALUE)):
        img, _ = ho.volume("golden", block)
        with torch.no_grad():
            Fv, P, hw = filt(img, return_intermediate=True)
        assert Fv.shape == img.shape and P.shape == img.shape[2:]
        out[f"F_{key}"] = Fv[0, 0].numpy()
        if block is None:
            out["P_plain"], out["hu_plain"] = P.numpy(), hw.numpy()
    path = os.path.join(GOLDEN_DIR, "hessian_enhance.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
