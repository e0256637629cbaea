#!/usr/bin/env python3
"""Generates tests/golden/refc/*.npz with the REFERENCE'S OWN C code: mex/nddwt.c, compiled unchanged into oracle/_ref/libnddwt_ref.so
(`make -C oracle ref`) and driven by oracle/ndwt_ref.py the way the MATLAB class drives nd_dwt_mex.

Unlike tests/golden/*.npz (written by our oracle, reproduced by the reference in tests/test_reference_c.py) these vectors are reference
output: x, arbitrary coefficients c, y = dec(x, level) and rec(c) for both pres_l2_norm settings, plus the metadata keys of the other
fixtures (sizes, level, wname).  One file holds the real case and one the complex case (`_r`, `_c`), which keeps every file below 1 MiB.
They travel to machines that have neither the reference nor the library: tests/test_reference_c.py holds every oracle restatement to
them, tests/test_gpu_reference_c.py the HIP kernels.
Run from the repository root, after the library is built:  python tests/golden/make_golden_refc.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import ndwt_oracle as orc  # noqa: E402
import ndwt_ref as ref  # noqa: E402

OUT = os.path.join(HERE, "refc")
CASES = {
    "d1_n37_db2_L3": dict(sizes=[37], wname="db2", level=3),
    "d1_n40_db10_L2": dict(sizes=[40], wname="db10", level=2),           # the shortest legal axis of the longest filter
    "d2_12x10_db1db3_L2": dict(sizes=[12, 10], wname=["db1", "db3"], level=2),
    "d3_10x9x8_db4_L3": dict(sizes=[10, 9, 8], wname="db4", level=3),
    "d4_5x6x4x5_mixed_L2": dict(sizes=[5, 6, 4, 5], wname=["db1", "db3", "db1", "db2"], level=2),
}


def generate(name, tag):
    """the arrays of fixture `name`_`tag` (tag 'r': real data, 'c': complex), computed by the compiled reference"""
    c = CASES[name]
    sizes, wname, level = c["sizes"], c["wname"], c["level"]
    d = len(sizes)
    rng = np.random.default_rng(sum(map(ord, name)) + (1000 if tag == "c" else 0))
    out = {"sizes": np.array(sizes), "level": np.array(level), "wname": np.array(wname if isinstance(wname, list) else [wname] * d)}
    x = rng.standard_normal(sizes)
    cc = rng.standard_normal(sizes + [orc.num_bands(d, level)])
    if tag == "c":
        x = x + 1j * rng.standard_normal(sizes)
        cc = cc + 1j * rng.standard_normal(cc.shape)
    out[f"x_{tag}"] = x
    out[f"c_{tag}"] = cc
    for l2 in (0, 1):
        out[f"y_{tag}_l2{l2}"] = ref.dec(x, wname, level, l2)
        out[f"rec_{tag}_l2{l2}"] = ref.rec(cc, wname, l2)
    return out


def main():
    os.makedirs(OUT, exist_ok=True)
    for name in CASES:
        for tag in ("r", "c"):
            out = generate(name, tag)
            path = os.path.join(OUT, f"{name}_{tag}.npz")
            np.savez_compressed(path, **out)
            print(f"{name}_{tag}", os.path.getsize(path) // 1024, "KiB")
            assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
