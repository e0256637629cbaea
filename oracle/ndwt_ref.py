"""ctypes front end of oracle/_ref/libnddwt_ref.so: the reference's own mex/nddwt.c, compiled unchanged against the plain DFT of
oracle/ref/ (`make -C oracle ref`) -- TEST INFRASTRUCTURE ONLY.  Like the other oracle files, the package never loads it.

dec() and rec() do what the MATLAB class does around its nd_dwt_mex call and nothing else (Functions/nd_dwt_3D.m:157-161,217-225 and the
1-D, 2-D and 4-D classes alike): fftn of the input over the data axes, the frequency-domain kernel of get_filters in its compute='mex'
form (1/N folded in, nd_dwt_3D.m:325-341; here NdDwtMat.get_filters of ndwt_oracle.py, a restatement), column-major split real and
imaginary planes, nd_dwt_dec_1level / nd_dwt_rec_1level at level 1 and nd_dwt_dec / nd_dwt_rec above it as nd_dwt_mex.c:90-98,141-148
chooses, and the real part for real input.  What is pinned that way is the C control flow of nddwt.c given the kernels: band slots, level
order, the conjugate in the synthesis, where 1/2^d goes.  The MATLAB side stays a restatement.

Array convention of ndwt_oracle.py: x has the MATLAB shape [n1, .., nd], coefficients [n1, .., nd, bands].
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

try:
    from .ndwt_oracle import NdDwtMat, level_from_bands, num_bands
except ImportError:                                    # imported as a plain module (tests put oracle/ on sys.path)
    from ndwt_oracle import NdDwtMat, level_from_bands, num_bands

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_ref", "libnddwt_ref.so")
_LIB = None


class FftwIodim(ctypes.Structure):                     # oracle/ref/fftw3.h
    _fields_ = [("n", ctypes.c_int), ("is_", ctypes.c_int), ("os", ctypes.c_int)]


def reference_dir() -> str:
    """where `make ref` looks for the reference checkout (oracle/Makefile: NDWT_REFERENCE)"""
    return os.environ.get("NDWT_REFERENCE", "/root/reference")


def available() -> bool:
    return os.path.exists(LIB_PATH)


def load():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not available():
        raise FileNotFoundError(f"{LIB_PATH}: build it with `make -C oracle ref` (needs the reference checkout)")
    L = ctypes.CDLL(LIB_PATH)
    dp, ip, i, vp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_void_p
    for name, extra in (("nd_dwt_dec_1level", []), ("nd_dwt_rec_1level", [i]), ("nd_dwt_dec", [i]), ("nd_dwt_rec", [i, i])):
        f = getattr(L, name)                           # (outR, outI, imageR, imageI, kernelR, kernelI, num_dims, dims, ...), nddwt.c:98,142,189,242
        f.restype = None
        f.argtypes = [dp] * 6 + [i, ip] + extra
    L.fftw_plan_guru_split_dft.restype = vp
    L.fftw_plan_guru_split_dft.argtypes = [i, ctypes.POINTER(FftwIodim), i, ctypes.POINTER(FftwIodim), dp, dp, dp, dp, ctypes.c_uint]
    L.fftw_execute_split_dft.restype = None
    L.fftw_execute_split_dft.argtypes = [vp, dp, dp, dp, dp]
    L.fftw_destroy_plan.restype = None
    L.fftw_destroy_plan.argtypes = [vp]
    _LIB = L
    return L


def _ptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _planes(a):
    """complex array -> (re, im): fresh column-major planes, flat (the C code overwrites its inputs)"""
    a = np.asarray(a, dtype=np.complex128)
    return np.array(a.real.reshape(-1, order="F"), dtype=np.float64), np.array(a.imag.reshape(-1, order="F"), dtype=np.float64)


def _kernel(wname, sizes, pres_l2_norm):
    return NdDwtMat(wname, sizes, pres_l2_norm, compute="mex").f_dec


def dec(x, wname, level, pres_l2_norm=0):
    """y = dec(x, level) of the class with compute = 'mex': [n1, .., nd] -> [n1, .., nd, bands]"""
    L = load()
    x = np.asarray(x)
    sizes, d = list(x.shape), x.ndim
    level = int(level)
    nb = num_bands(d, level)
    imr, imi = _planes(np.fft.fftn(x))                                          # nd_dwt_3D.m:157
    kr, ki = _planes(_kernel(wname, sizes, pres_l2_norm))
    outr, outi = np.zeros(x.size * nb), np.zeros(x.size * nb)
    dims = (ctypes.c_int * d)(*sizes)
    if level == 1:                                                              # nd_dwt_mex.c:90-98
        L.nd_dwt_dec_1level(_ptr(outr), _ptr(outi), _ptr(imr), _ptr(imi), _ptr(kr), _ptr(ki), d, dims)
    else:
        L.nd_dwt_dec(_ptr(outr), _ptr(outi), _ptr(imr), _ptr(imi), _ptr(kr), _ptr(ki), d, dims, level)
    y = (outr + 1j * outi).reshape(sizes + [nb], order="F")
    return np.ascontiguousarray(y.real) if np.isrealobj(x) else np.ascontiguousarray(y)   # :190-192


def rec(c, wname, pres_l2_norm=0):
    """x = rec(c) of the class with compute = 'mex': [n1, .., nd, bands] -> [n1, .., nd]"""
    L = load()
    c = np.asarray(c)
    sizes, d = list(c.shape[:-1]), c.ndim - 1
    level = level_from_bands(d, c.shape[-1])                                    # :217
    imr, imi = _planes(np.fft.fftn(c, axes=tuple(range(d))))                    # :220
    kr, ki = _planes(_kernel(wname, sizes, pres_l2_norm))
    numel = int(np.prod(sizes))
    outr, outi = np.zeros(numel), np.zeros(numel)                               # nd_dwt_rec_1level accumulates with += (nddwt.c:170-171)
    dims = (ctypes.c_int * d)(*sizes)
    l2 = int(bool(pres_l2_norm))
    if level == 1:                                                              # nd_dwt_mex.c:141-148
        L.nd_dwt_rec_1level(_ptr(outr), _ptr(outi), _ptr(imr), _ptr(imi), _ptr(kr), _ptr(ki), d, dims, l2)
    else:
        L.nd_dwt_rec(_ptr(outr), _ptr(outi), _ptr(imr), _ptr(imi), _ptr(kr), _ptr(ki), d, dims, level, l2)
    y = (outr + 1j * outi).reshape(sizes, order="F")
    return np.ascontiguousarray(y.real) if np.isrealobj(c) else np.ascontiguousarray(y)   # :248-250


def shim_dft(a, rank, howmany=1, inverse=False):
    """the DFT of oracle/ref/fftw_split_dft.c over the first `rank` axes of `a` ([n1, .., n_rank] or [n1, .., n_rank, howmany]), called the
    way nddwt.c:15-61 plans it: column-major strides, one howmany dimension of stride numel, in place.  inverse = the pointer-swapped call
    of nddwt.c:128,164, which gives the unnormalised inverse DFT"""
    L = load()
    a = np.asarray(a, dtype=np.complex128)
    sizes = list(a.shape[:rank])
    numel = int(np.prod(sizes))
    assert a.size == numel * howmany
    re, im = _planes(a)
    dims = (FftwIodim * rank)()
    stride = 1
    for k, n in enumerate(sizes):
        dims[k].n, dims[k].is_, dims[k].os = n, stride, stride
        stride *= n
    hm = (FftwIodim * 1)()
    hm[0].n, hm[0].is_, hm[0].os = howmany, numel, numel
    first, second = (im, re) if inverse else (re, im)
    plan = L.fftw_plan_guru_split_dft(rank, dims, 1, hm, _ptr(first), _ptr(second), _ptr(first), _ptr(second), 1 << 6)
    assert plan
    L.fftw_execute_split_dft(plan, _ptr(first), _ptr(second), _ptr(first), _ptr(second))
    L.fftw_destroy_plan(plan)
    return (re + 1j * im).reshape(a.shape, order="F")
