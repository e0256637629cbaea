"""What tests/test_emulated_select.py and tests/test_gpu_select.py share: the contents of a band, the ranks of a call and the two
checks -- real data bit for bit against numpy, complex data by counting magnitudes on either side of the value.

A band's contents (N elements; `rdt` the scalar type):
  gauss      standard normal
  equal      every element +-1.5: every count in one bin at every digit
  split      two distinct values, split exactly at the median (N odd: the lower value holds it)
  lowdigit   values that differ only in the lowest digit of the key (float: 10 bits, double: 9)
  highdigit  values that differ only in the highest digit (the top 11 bits: exponent, and for float two mantissa bits; no inf / NaN)
  special    zeros of both signs, denormals, one inf and one NaN among normal values (N >= 16)
Complex bands take gauss, equal (|c| = 2.5 exactly, with varying signs and parts), split and zeros (half the elements zero, of
either sign).
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

REAL_CONTENTS = ("gauss", "equal", "split", "lowdigit", "highdigit", "special")
COMPLEX_CONTENTS = ("gauss", "equal", "split", "zeros")
KINDS = {"f32": (np.float32, False), "c64": (np.float32, True), "f64": (np.float64, False), "c128": (np.float64, True)}


def build_shim(tmp_path_factory):
    """tests/select/bandselect_shim.cpp as a shared object: the host-side decisions of csrc/ndwt_select.h, with their argument types"""
    if not shutil.which("g++"):
        pytest.skip("no g++ to compile tests/select/bandselect_shim.cpp")
    out = str(tmp_path_factory.mktemp("select_band") / "libbandselect_shim.so")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", os.path.join(HERE, "select", "bandselect_shim.cpp"), "-o", out],
                   check=True)
    lib = ctypes.CDLL(out)
    lib.sel_select_vec.argtypes = [ctypes.c_ulonglong, ctypes.c_longlong, ctypes.c_int]
    lib.sel_select_grid.argtypes = [ctypes.c_longlong] + [ctypes.c_int] * 4
    lib.sel_select_grid.restype = ctypes.c_longlong
    lib.sel_select_fits.argtypes = [ctypes.c_longlong]
    return lib


def _bits(rdt):
    return (np.uint32, 32, 10) if rdt == np.float32 else (np.uint64, 64, 9)


def real_band(rdt, N, content, seed):
    rng = np.random.default_rng(seed)
    udt, keybits, lowbits = _bits(rdt)
    sign = np.where(rng.random(N) < 0.5, -1.0, 1.0).astype(rdt)
    if content == "gauss":
        return rng.standard_normal(N).astype(rdt)
    if content == "equal":
        return (sign * rdt(1.5)).astype(rdt)
    if content == "split":
        v = np.where(np.arange(N) < (N + 1) // 2, rdt(0.75), rdt(3.25)).astype(rdt)
        return (rng.permutation(v) * sign).astype(rdt)
    if content == "lowdigit":
        base = np.array([1.25], dtype=rdt).view(udt)[0]
        key = (base + rng.integers(0, 1 << lowbits, N).astype(udt)).astype(udt)
        return (key.view(rdt) * sign).astype(rdt)
    if content == "highdigit":
        low = np.array([1.0 + 1.0 / 3.0], dtype=rdt).view(udt)[0] & udt((1 << (keybits - 11)) - 1)
        top = rng.integers(1, (255 << 2) if rdt == np.float32 else 0x3FF, N).astype(udt)   # below the all-ones exponent
        key = ((top << udt(keybits - 11)) | low).astype(udt)
        return (key.view(rdt) * sign).astype(rdt)
    if content == "special":
        assert N >= 16
        v = rng.standard_normal(N).astype(rdt)
        tiny = np.finfo(rdt).tiny
        v[:10] = [0.0, -0.0, 0.0, -0.0, tiny / 4, -tiny / 8, np.nextafter(rdt(0), rdt(1)), -tiny / 2, np.inf, np.nan]
        return rng.permutation(v).astype(rdt)
    raise ValueError(content)


def complex_band(rdt, N, content, seed):
    """interleaved (re, im): 2 N scalars"""
    rng = np.random.default_rng(seed)
    if content == "gauss":
        re, im = rng.standard_normal(N), rng.standard_normal(N)
    elif content == "equal":
        ph = rng.integers(0, 4, N)
        re, im = np.where(ph % 2 == 0, 1.5, 2.0) * np.where(ph < 2, 1, -1), np.where(ph % 2 == 0, 2.0, 1.5) * np.where(rng.random(N) < 0.5, 1, -1)
    elif content == "split":
        big = rng.permutation(np.arange(N) >= (N + 1) // 2)
        re, im = np.where(big, 3.0, 0.5) * np.where(rng.random(N) < 0.5, 1, -1), np.where(big, -4.0, 0.25)
    elif content == "zeros":
        z = rng.permutation(np.arange(N) < (N + 1) // 2)
        re, im = np.where(z, np.where(rng.random(N) < 0.5, 0.0, -0.0), rng.standard_normal(N)), np.where(z, -0.0, rng.standard_normal(N))
    else:
        raise ValueError(content)
    out = np.empty(2 * N, dtype=rdt)
    out[0::2] = re
    out[1::2] = im
    return out


def rank_sets(N):
    """the calls made on every band: the ends and the two middle ranks in one call, and one rank twice in one call"""
    return [[0, N - 1, (N - 1) // 2, N // 2], [N // 3, N // 3]]


def check_real(y, ks, got, what=""):
    """values[i] == np.partition(np.abs(y), k)[k] bit for bit; a NaN is the last order statistic, and the others are those of the band
    without it"""
    a = np.abs(y)
    want = np.sort(a)[np.asarray(ks)]                            # (== np.partition(a, k)[k]: numpy sorts a NaN last)
    got = np.asarray(got, dtype=np.float64)
    w64 = want.astype(np.float64)
    same = (got.view(np.uint64) == w64.view(np.uint64)) | (np.isnan(got) & np.isnan(w64))
    assert same.all(), f"{what}: ranks {list(ks)}: got {got!r}, want {w64!r}"
    nan = np.isnan(a)
    if nan.any():
        clean = np.sort(a[~nan])
        for k, g in zip(ks, got):
            if k < clean.size:
                assert g == np.float64(clean[k]), f"{what}: rank {k} moved with the NaN in the band"
            else:
                assert np.isnan(g), f"{what}: rank {k} is among the NaNs"


def check_complex(y, ks, got, what=""):
    """count(m < v (1 - eps)) <= k < count(m <= v (1 + eps)), m = hypot(re, im) in double, eps = 4 machine epsilons of the scalar
    type: the device's magnitude takes at most three roundings (product or FMA, sum, square root), under 2 ulp, and the margin is twice that"""
    m = np.hypot(y[0::2].astype(np.float64), y[1::2].astype(np.float64))
    eps = 4 * float(np.finfo(y.dtype).eps)
    for k, v in zip(ks, np.asarray(got, dtype=np.float64)):
        below, upto = int((m < v * (1 - eps)).sum()), int((m <= v * (1 + eps)).sum())
        assert below <= k < upto, f"{what}: rank {k}: value {v!r} has {below} magnitudes below and {upto} up to it"
