"""What the tests of the per-item calls share (tests/test_emulated_select_items.py, tests/test_gpu_items.py): the items of a band, the
ranks of a call and the check of a result against numpy, item by item.

An item is one signal of a batch, one image / volume of a stack, one block of interleaved samples: N elements that lie together, item j
behind item j - 1.  Item j is a draw of its own scaled by (j + 1), so a result that belongs to another item is far off.  With three
items or more, item 1 is all-equal (every count in one bin at every digit) and item 2 holds one NaN: it must be that item's last order
statistic and must leave the statistics of its neighbours -- and its own lower ranks -- alone.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from select_cases import KINDS, check_complex, check_real, complex_band, real_band

HERE = os.path.dirname(os.path.abspath(__file__))


def build_named_shim(tmp_path_factory, name):
    """tests/select/<name>.cpp as a shared object: host-side decisions of csrc/ndwt_select.h"""
    if not shutil.which("g++"):
        pytest.skip(f"no g++ to compile tests/select/{name}.cpp")
    out = str(tmp_path_factory.mktemp(name) / f"lib{name}.so")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", os.path.join(HERE, "select", f"{name}.cpp"), "-o", out], check=True)
    return ctypes.CDLL(out)


def build_items_shim(tmp_path_factory):
    """tests/select/items_shim.cpp with its argument types"""
    lib = build_named_shim(tmp_path_factory, "items_shim")
    lib.sel_items_one_launch.argtypes = [ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_int]
    lib.sel_items_route_const.restype = ctypes.c_longlong
    lib.sel_shrink_items_chunks.argtypes = [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int]
    lib.sel_shrink_items_chunks.restype = ctypes.c_longlong
    return lib


def item_ranks(N):
    """the calls made on every band: the ends and the two middle ranks in one call, and one rank twice in one call (N: elements of ONE item)"""
    return [[0, N - 1, (N - 1) // 2, N // 2], [N // 3, N // 3]]


def items_band(kind, items, N, seed, special=True):
    """[items, N * comp] scalars in kernel form (complex: interleaved)"""
    rdt, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    make = complex_band if cplx else real_band
    out = np.empty((items, N * comp), dtype=rdt)
    for j in range(items):
        content = "equal" if (special and items >= 3 and j == 1) else "gauss"
        out[j] = make(rdt, N, content, seed + 7919 * j) * rdt(j + 1)
    if special and items >= 3:
        out[2, (N // 2) * comp] = np.nan                       # (complex: the real part of one element)
    return out


def check_items(kind, data, ks, got, what=""):
    """got[j] against item j alone: real data bit for bit (select_cases.check_real), complex data by counting (check_complex); an item with
    a NaN: the ranks below its count of numbers are those of the item without it, the others are NaN"""
    rdt, cplx = KINDS[kind]
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == (data.shape[0], len(ks)), (what, got.shape)
    for j in range(data.shape[0]):
        w = f"{what} item {j}"
        if not cplx:
            check_real(data[j], ks, got[j], w)
            continue
        bad = np.isnan(data[j][0::2]) | np.isnan(data[j][1::2])
        if not bad.any():
            check_complex(data[j], ks, got[j], w)
            continue
        clean = data[j].reshape(-1, 2)[~bad].reshape(-1)
        low = [i for i, k in enumerate(ks) if k < clean.size // 2]
        check_complex(clean, [ks[i] for i in low], got[j][low], w)
        for i, k in enumerate(ks):
            if i not in low:
                assert np.isnan(got[j][i]), f"{w}: rank {k} is among the NaNs, got {got[j][i]!r}"

