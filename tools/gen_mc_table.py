#!/usr/bin/env python3
"""Writes fissure-segmentation_amd/csrc/mc_table.h from the generator in fissure-segmentation_amd/_mc_table.py (loaded by path:
the generator has no dependencies, so this runs before the library is built).  `--check` only compares."""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fissure-segmentation_amd")


def main():
    spec = importlib.util.spec_from_file_location("_mc_table", os.path.join(PKG, "_mc_table.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    path = os.path.join(PKG, "csrc", "mc_table.h")
    text = gen.header()
    if "--check" in sys.argv[1:]:
        same = os.path.exists(path) and open(path).read() == text
        print("mc_table.h is", "up to date" if same else "STALE")
        return 0 if same else 1
    with open(path, "w") as f:
        f.write(text)
    print(f"wrote {path}: {sum(len(t) for t in gen.TRIANGLES)} triangles over 256 cases, at most {gen.MAX_TRIANGLES} per case")
    return 0


if __name__ == "__main__":
    sys.exit(main())
