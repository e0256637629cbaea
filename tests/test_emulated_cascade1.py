"""The cascaded 1-D kernels of a batched plan (Fwd1C / Inv1C of csrc/ndwt_device_1d.h) emulated on the host
(tests/emu/ndwt_emu_cascade1.cpp: the kernel bodies compiled as plain C++, every lane of a wave run in turn) against the numpy oracle,
signal by signal -- before any of it reaches a GPU.  Four kinds (float, complex64, double, complex128) x both directions.

The cases: two segments whose second one is partial and wraps around the row (n comp = WX + 32); a row shorter than one wave's span
(n comp = 64 with db4: a wave wraps it four times); five signals of one segment each, so that the last workgroup has idle waves; db1;
two, three and four levels.  Tolerances are those of tests/test_gpu_parity.py: 1e-12 (double), 2e-6 (single) relative for dec, and
2 TOL max(|want|, |c|) for rec.

The same cases run once more as a stand-alone program built with AddressSanitizer and UBSan (ndwt_emu_cascade1_main.cpp, every buffer a
heap block of exactly its size): a child process with nothing preloaded, which must exit 0.
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
KINDS = {"f32": (np.float32, False), "c64": (np.float32, True), "f64": (np.float64, False), "c128": (np.float64, True)}
PARTS = range(5)                                              # EMU_C1_PART: 0 the entry point, 1 .. 4 the kinds


def tile_width(inverse, f64, ew, L, nlev):
    """Fwd1C::WX / Inv1C::WX: the lanes valid at every level, in whole 128-byte lines"""
    LH, RH = (L // 2, L // 2 - 1) if inverse else (L // 2 - 1, L // 2)
    lpl = 4 if f64 else 8
    return 4 * ((64 - nlev * ((LH * ew + 3) // 4 + (RH * ew + 3) // 4)) // lpl * lpl)


# (id, wavelet, levels, signals, scalars per row or None = WX + 32 of the kind and direction)
SHAPES = [
    ("two-segments-db4-3", "db4", 3, 3, None),
    ("short-row-db4-4", "db4", 4, 2, 64),
    ("five-signals-db2-2", "db2", 2, 5, 96),
    ("db1-3", "db1", 3, 3, None),
    ("db3-4", "db3", 4, 2, None),
]
CASES = [(f"{kind}-{sid}", kind, wn, nlev, K, row) for kind in KINDS for sid, wn, nlev, K, row in SHAPES]


def _sources():
    return [os.path.join(EMU, "ndwt_emu_cascade1.cpp"), os.path.join(EMU, "ndwt_emu.cpp"), os.path.join(CSRC, "ndwt_device_1d.h"),
            os.path.join(CSRC, "ndwt_device.h"), os.path.join(CSRC, "ndwt_wave_row.h"), os.path.join(CSRC, "ndwt_geom.h"), os.path.join(CSRC, "ndwt_fused_tile.h"),
            os.path.join(CSRC, "ndwt_taps_host.h")]


def _build(tag, flags, link_flags, out, extra=()):
    """the parts of ndwt_emu_cascade1.cpp (and `extra` sources) compiled in parallel into tests/emu/build, linked to `out`; as make
    would, only what is older than its sources is rebuilt"""
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain is needed to build the host emulator")
    bdir = os.path.join(EMU, "build")
    os.makedirs(bdir, exist_ok=True)
    newest = max(os.path.getmtime(f) for f in _sources() + list(extra))
    jobs = [(os.path.join(bdir, f"cascade1_{tag}_{p}.o"), [f"-DEMU_C1_PART={p}", _sources()[0]]) for p in PARTS]
    jobs += [(os.path.join(bdir, f"cascade1_{tag}_{os.path.basename(e)}.o"), [e]) for e in extra]

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
    so = _build("plain", ["-O1"], ["-shared", "-fPIC"], os.path.join(EMU, "libndwt_emu_cascade1.so"))
    lib = ctypes.CDLL(so)
    lib.ndwt_emu1_cascade.restype = ctypes.c_int
    lib.ndwt_emu1_cascade.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p] * 2 + [ctypes.c_longlong] * 2 + [ctypes.c_void_p] * 2
    return lib


def _per_part(f, a):
    """the oracle on a complex array: the filters are real, so the transform of the real and of the imaginary part"""
    return f(a.real) + 1j * f(a.imag) if np.iscomplexobj(a) else f(a)


_MADE = {}


def make_case(cid, kind, wn, nlev, K, row, inverse, l2=1):
    """(L, lo, hi, kernel-order input, oracle output [n, K(, bands)], input [n, K(, bands)], scalars per row): the input rounded to the
    kind's precision, the oracle in double, signal by signal"""
    key = (cid, inverse)
    if key not in _MADE:
        rdt, cplx = KINDS[kind]
        comp = 2 if cplx else 1
        cdt = (np.complex64 if rdt == np.float32 else np.complex128) if cplx else rdt
        L = len(orc.wave_filters(wn)[0])
        if row is None:
            row = tile_width(inverse, rdt == np.float64, comp, L, nlev) + 32
        assert row % 4 == 0 and row % comp == 0 and row >= 8 * L
        n = row // comp
        rng = np.random.default_rng(zlib.crc32(repr((cid, wn, nlev, K, row, inverse)).encode()))
        shape = (n, K) + ((1 + nlev,) if inverse else ())
        a = rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if cplx else 0)
        a = a.astype(cdt).astype(np.complex128 if cplx else np.float64)
        one = (lambda v: orc.spatial_rec(v, [wn], l2)) if inverse else (lambda v: orc.spatial_dec(v, [wn], nlev, l2))
        want = np.stack([_per_part(one, a[:, k]) for k in range(K)], axis=1)
        t = kernel_taps(wn, l2)
        lo, hi = np.zeros(20), np.zeros(20)
        lo[:L], hi[:L] = (t["syn_lo"], t["syn_hi"]) if inverse else (t["ana_lo"], t["ana_hi"])
        _MADE[key] = (L, lo, hi, np.ascontiguousarray(to_kernel_order(a).astype(cdt)), want, a, row)
    return _MADE[key]


def _bound(kind, inverse, want, a):
    tol = TOL["single" if KINDS[kind][0] == np.float32 else "double"]
    return 2 * tol * max(np.abs(want).max(), np.abs(a).max()) if inverse else tol * np.abs(want).max()


@pytest.mark.parametrize("cid,kind,wn,nlev,K,row", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("inverse", [False, True], ids=["dec", "rec"])
def test_emulated_cascade_of_the_kind(emu, cid, kind, wn, nlev, K, row, inverse):
    rdt, cplx = KINDS[kind]
    L, lo, hi, src, want, a, row = make_case(cid, kind, wn, nlev, K, row, inverse)
    n = src.shape[-1]
    out = np.full(((K, n) if inverse else (1 + nlev, K, n)), np.nan, dtype=src.dtype)
    rc = emu.ndwt_emu1_cascade(int(inverse), int(rdt == np.float64), 2 if cplx else 1, L, nlev, src.ctypes.data, out.ctypes.data, row, K,
                               lo.ctypes.data, hi.ctypes.data)
    assert rc == 0
    got = np.transpose(out)
    assert np.isfinite(got).all()                             # every element of every band was written
    err, bound = np.abs(got - want).max(), _bound(kind, inverse, want, a)
    print(f"{cid} {'rec' if inverse else 'dec'}: row {row} scalars, max error {err:.3g}, bound {bound:.3g}")
    assert err <= bound


def test_the_emulator_refuses_what_is_not_an_instance(emu):
    x = np.zeros(256, dtype=np.float32)
    y = np.zeros(5 * 256, dtype=np.float32)
    t = np.zeros(20)
    for L, nlev, row in ((10, 2, 256), (8, 5, 256), (8, 1, 256), (8, 2, 254)):
        assert emu.ndwt_emu1_cascade(0, 0, 1, L, nlev, x.ctypes.data, y.ctypes.data, row, 1, t.ctypes.data, t.ctypes.data) == -1


def test_the_cases_run_clean_under_address_and_ub_sanitizers(tmp_path):
    """the stand-alone program (its own main, -fsanitize=address,undefined) on every case above, as a child process"""
    san = ["-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    prog = _build("asan", san, ["-fsanitize=address,undefined"], os.path.join(EMU, "build", "ndwt_emu_cascade1_asan"),
                  extra=[os.path.join(EMU, "ndwt_emu_cascade1_main.cpp")])
    blob, ncases = [], 0
    for cid, kind, wn, nlev, K, row in CASES:
        rdt, cplx = KINDS[kind]
        for inverse in (False, True):
            L, lo, hi, src, want, a, r = make_case(cid, kind, wn, nlev, K, row, inverse)
            blob.append(struct.pack("<7i", int(inverse), int(rdt == np.float64), 2 if cplx else 1, L, nlev, r, K))
            blob.append(lo.astype("<f8").tobytes() + hi.astype("<f8").tobytes() + struct.pack("<d", float(_bound(kind, inverse, want, a))))
            blob.append(src.tobytes())
            blob.append(np.ascontiguousarray(to_kernel_order(want).astype(src.dtype)).tobytes())
            ncases += 1
    path = tmp_path / "cases.bin"
    path.write_bytes(struct.pack("<i", ncases) + b"".join(blob))
    r = subprocess.run([prog, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert f"{ncases} cases ok" in r.stdout
