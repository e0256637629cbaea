"""The cascaded 2-D kernels (Fwd2C / Inv2C of csrc/ndwt_device.h) on complex64, double and complex128 data, emulated on the host
(tests/emu/ndwt_emu_cascade2_kinds.cpp: the kernel bodies compiled as plain C++, every lane of a wave run in turn) against the numpy
oracle -- before any of it reaches a GPU.

The cases, per kind: two tiles along x whose second one is partial and wraps around the row; chunks shorter than the march-in, so that
every level starts in another chunk's rows; mixed wavelets (db2, db3); db1; two and three levels; for complex64 also two rows of band
loads in flight.  Tolerances are those of tests/test_gpu_parity.py: 1e-12 (double), 2e-6 (single) relative for dec, and
2 TOL max(|want|, |c|) for rec.

The same cases run once more as a stand-alone program built with AddressSanitizer and UBSan (ndwt_emu_cascade2_kinds_main.cpp, every
buffer a heap block of exactly its size): a child process with nothing preloaded, which must exit 0.
"""
import concurrent.futures
import ctypes
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import ndwt_oracle as orc
from helpers import kernel_taps, to_kernel_order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "non-decimated_wavelets_amd", "csrc")
CXX = "/opt/rocm/lib/llvm/bin/clang++"
TOL = {"double": 1e-12, "single": 2e-6}                       # tests/test_gpu_parity.py
KINDS = {"c64": (np.float32, True), "f64": (np.float64, False), "c128": (np.float64, True)}
PARTS = range(7)                                              # EMU_KINDS_PART: 0 the entry point, 1 .. 6 kind x direction

# (id, sizes in elements, wavelets, levels, rows per wave, rows of band loads in flight)
SHAPES = [
    ("two-tiles-short-chunks", {"c64": (128, 50), "f64": (256, 50), "c128": (128, 50)}, ("db4", "db4"), 3, 17, 1),   # march-in 21 rows > 17
    ("mixed-db2-db3", {"c64": (132, 31), "f64": (260, 31), "c128": (132, 31)}, ("db2", "db3"), 2, 8, 1),             # second tile mostly outside
    ("db1", {"c64": (32, 30), "f64": (32, 30), "c128": (32, 30)}, ("db1", "db1"), 3, 7, 1),
    ("db3-two-levels", {"c64": (128, 38), "f64": (256, 38), "c128": (128, 38)}, ("db3", "db3"), 2, 13, 2),
    ("db2-three-levels-one-chunk", {"c64": (128, 20), "f64": (240, 20), "c128": (128, 20)}, ("db2", "db4"), 3, 0, 1),
]
CASES = [(f"{kind}-{sid}", kind, sizes[kind], wn, nlev, ychunk, depth if kind == "c64" else 1)
         for kind in KINDS for sid, sizes, wn, nlev, ychunk, depth in SHAPES]


def _sources():
    return [os.path.join(EMU, "ndwt_emu_cascade2_kinds.cpp"), os.path.join(EMU, "ndwt_emu.cpp"), os.path.join(CSRC, "ndwt_device.h"),
            os.path.join(CSRC, "ndwt_wave_row.h"), os.path.join(CSRC, "ndwt_geom.h"), os.path.join(CSRC, "ndwt_fused_tile.h"),
            os.path.join(CSRC, "ndwt_taps_host.h")]


def _build(tag, flags, link_flags, out, extra=()):
    """the parts of ndwt_emu_cascade2_kinds.cpp (and `extra` sources) compiled in parallel into tests/emu/build, linked to `out`; as make
    would, only what is older than its sources is rebuilt"""
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain is needed to build the host emulator")
    bdir = os.path.join(EMU, "build")
    os.makedirs(bdir, exist_ok=True)
    newest = max(os.path.getmtime(f) for f in _sources() + list(extra))
    jobs = [(os.path.join(bdir, f"kinds_{tag}_{p}.o"), [f"-DEMU_KINDS_PART={p}", _sources()[0]]) for p in PARTS]
    jobs += [(os.path.join(bdir, f"kinds_{tag}_{os.path.basename(e)}.o"), [e]) for e in extra]

    def compile_one(job):
        obj, src = job
        if not os.path.exists(obj) or os.path.getmtime(obj) < newest:
            subprocess.check_call([CXX, "-std=c++17", "-fPIC", f"-I{CSRC}"] + flags + ["-c"] + src + ["-o", obj])
        return obj
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        objs = list(pool.map(compile_one, jobs))
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(o) for o in objs):
        subprocess.check_call([CXX] + link_flags + objs + ["-o", out])
    return out


@pytest.fixture(scope="module")
def emu():
    so = _build("plain", ["-O1"], ["-shared", "-fPIC"], os.path.join(EMU, "libndwt_emu_cascade2_kinds.so"))
    lib = ctypes.CDLL(so)
    lib.ndwt_emu2_cascade_kinds.restype = ctypes.c_int
    lib.ndwt_emu2_cascade_kinds.argtypes = [ctypes.c_int] * 6 + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2 + [ctypes.c_double, ctypes.c_int]
    return lib


def _taps(wn, l2, inverse):
    Lp = max(len(orc.wave_filters(w)[0]) for w in wn)
    lo, hi = np.zeros((3, 20)), np.zeros((3, 20))
    for ax in range(2):
        t = kernel_taps(wn[ax], l2, Lp)
        lo[ax, :Lp], hi[ax, :Lp] = (t["syn_lo"], t["syn_hi"]) if inverse else (t["ana_lo"], t["ana_hi"])
    return Lp, lo, hi


def _per_part(f, a):
    """the oracle on a complex array: the filters are real, so the transform of the real and of the imaginary part"""
    return f(a.real) + 1j * f(a.imag) if np.iscomplexobj(a) else f(a)


_MADE = {}


def make_case(cid, kind, sizes, wn, nlev, inverse, l2=1):
    """(Lp, lo, hi, kernel-order input, oracle output in MATLAB shape, input in MATLAB shape): the input rounded to the kind's precision,
    the oracle in double"""
    key = (cid, inverse)
    if key not in _MADE:
        rdt, cplx = KINDS[kind]
        cdt = (np.complex64 if rdt == np.float32 else np.complex128) if cplx else rdt
        rng = np.random.default_rng(zlib.crc32(repr((cid, sizes, wn, nlev, inverse)).encode()))
        shape = tuple(sizes) + ((1 + 3 * nlev,) if inverse else ())
        a = rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if cplx else 0)
        a = a.astype(cdt).astype(np.complex128 if cplx else np.float64)
        want = _per_part((lambda v: orc.spatial_rec(v, list(wn), l2)) if inverse else (lambda v: orc.spatial_dec(v, list(wn), nlev, l2)), a)
        Lp, lo, hi = _taps(wn, l2, inverse)
        _MADE[key] = (Lp, lo, hi, np.ascontiguousarray(to_kernel_order(a).astype(cdt)), want, a)
    return _MADE[key]


def _bound(kind, inverse, want, a):
    tol = TOL["single" if KINDS[kind][0] == np.float32 else "double"]
    return 2 * tol * max(np.abs(want).max(), np.abs(a).max()) if inverse else tol * np.abs(want).max()


@pytest.mark.parametrize("cid,kind,sizes,wn,nlev,ychunk,depth", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("inverse", [False, True], ids=["dec", "rec"])
def test_emulated_cascade_of_the_kind(emu, cid, kind, sizes, wn, nlev, ychunk, depth, inverse):
    rdt, cplx = KINDS[kind]
    Lp, lo, hi, src, want, a = make_case(cid, kind, sizes, wn, nlev, inverse)
    n2, n1 = src.shape[-2:]
    out = np.full(((n2, n1) if inverse else (1 + 3 * nlev, n2, n1)), np.nan, dtype=src.dtype)
    rc = emu.ndwt_emu2_cascade_kinds(int(inverse), int(rdt == np.float64), 2 if cplx else 1, Lp, nlev, depth if inverse else 1, src.ctypes.data, out.ctypes.data,
                                     n1 * (2 if cplx else 1), n2, ychunk, lo.ctypes.data, hi.ctypes.data, 0.0, 0)
    assert rc == 0
    got = np.transpose(out)
    assert np.isfinite(got).all()
    err, bound = np.abs(got - want).max(), _bound(kind, inverse, want, a)
    print(f"{cid} {'rec' if inverse else 'dec'}: max error {err:.3g}, bound {bound:.3g}")
    assert err <= bound


def test_emulated_cascade_shrinks_the_magnitude_of_complex_coefficients(emu):
    """the thresholding fused into Inv2C's loads: soft shrinkage of |re + i im| for interleaved complex data, of |v| for real data"""
    for kind, sizes in (("c64", (128, 38)), ("c128", (128, 38)), ("f64", (256, 38))):
        rdt, cplx = KINDS[kind]
        wn, nlev = ("db2", "db2"), 2
        Lp, lo, hi, src, _, c = make_case(f"{kind}-shrink", kind, sizes, wn, nlev, True)
        thr = 0.7
        m = np.abs(c)
        cs = c * np.where(m > thr, (m - thr) / np.where(m > 0, m, 1.0), 0.0)
        cs[..., 0] = c[..., 0]
        want = _per_part(lambda v: orc.spatial_rec(v, list(wn), 1), cs)
        n2, n1 = src.shape[-2:]
        out = np.full((n2, n1), np.nan, dtype=src.dtype)
        rc = emu.ndwt_emu2_cascade_kinds(1, int(rdt == np.float64), 2 if cplx else 1, Lp, nlev, 1, src.ctypes.data, out.ctypes.data,
                                         n1 * (2 if cplx else 1), n2, 11, lo.ctypes.data, hi.ctypes.data, thr, 0)
        assert rc == 0
        assert np.abs(np.transpose(out) - want).max() <= _bound(kind, True, want, c), kind


def test_the_cases_run_clean_under_address_and_ub_sanitizers(tmp_path):
    """the stand-alone program (its own main, -fsanitize=address,undefined) on every case above, as a child process"""
    san = ["-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    prog = _build("asan", san, ["-fsanitize=address,undefined"], os.path.join(EMU, "build", "ndwt_emu_cascade2_kinds_asan"),
                  extra=[os.path.join(EMU, "ndwt_emu_cascade2_kinds_main.cpp")])
    blob, n = [], 0
    for cid, kind, sizes, wn, nlev, ychunk, depth in CASES:
        rdt, cplx = KINDS[kind]
        for inverse in (False, True):
            Lp, lo, hi, src, want, a = make_case(cid, kind, sizes, wn, nlev, inverse)
            n2, n1 = src.shape[-2:]
            blob.append(struct.pack("<9i", int(inverse), int(rdt == np.float64), 2 if cplx else 1, Lp, nlev, depth if inverse else 1, n1 * (2 if cplx else 1), n2, ychunk))
            blob.append(lo.astype("<f8").tobytes() + hi.astype("<f8").tobytes() + struct.pack("<d", float(_bound(kind, inverse, want, a))))
            blob.append(src.tobytes())
            blob.append(np.ascontiguousarray(to_kernel_order(want).astype(src.dtype)).tobytes())
            n += 1
    path = tmp_path / "cases.bin"
    path.write_bytes(struct.pack("<i", n) + b"".join(blob))
    r = subprocess.run([prog, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert f"{n} cases ok" in r.stdout
