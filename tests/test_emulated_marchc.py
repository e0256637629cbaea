"""The cascaded march of one strided axis (FwdMC / InvMC of csrc/ndwt_device_axis.h) emulated on the host (tests/emu/ndwt_emu_marchc.cpp:
the kernel bodies compiled as plain C++, every thread of a workgroup run in turn) against the numpy oracle -- slice one inner index of
one item, transform, compare -- before any of it reaches a GPU.  Four data kinds (interleaved complex is the factor 2 in the inner
block) x both directions x (db1, 3 levels), (db2, 2), (db4, 3), (db4, 4), wherever the library's table has the instance.

Shapes [scalars of the inner block, n, items]:
  * [4, L, 1]      one group of 4 scalars, the axis as short as the filter: the march-in of NLEV (L - 1) planes wraps it more than twice;
  * [12, 19, 3]    one chunk per item;
  * [12, 19, 3]    chunks of 7 planes: three per item, the last partial, the march-in wrapping inside the item -- a thread that read
                   the neighbouring item instead misses the oracle;
  * [1028, 9, 1]   257 groups: a second workgroup with 255 idle threads.
Tolerances are those of tests/test_gpu_parity.py: 1e-12 (double), 2e-6 (single) relative for dec, and 2 TOL max(|want|, |c|) for rec.

The same cases run once more as a stand-alone program built with AddressSanitizer and UBSan (ndwt_emu_marchc_main.cpp, every buffer a
heap block of exactly its size): a child process with nothing preloaded, which must exit 0.
"""
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


def instantiated(inverse, f64, L, nlev):
    """ndwt_fused_list.h: the CascadeMInstance table"""
    return L in (2, 4, 6, 8) and 2 <= nlev <= 4 and not (inverse and f64 and L == 8 and nlev >= 3)


WAVELETS = [("db1", 3), ("db2", 2), ("db4", 3), ("db4", 4)]
# (id, scalars of the inner block, n or None = the tap length, items, planes per chunk or 0 = the whole axis)
SHAPES = [("short-axis", 4, None, 1, 0), ("one-chunk", 12, 19, 3, 0), ("chunks-of-7", 12, 19, 3, 7), ("two-blocks", 1028, 9, 1, 0)]
CASES = [(f"{kind}-{wn}-{nlev}-{sid}", kind, wn, nlev, inner, n, K, chunk)
         for kind in KINDS for wn, nlev in WAVELETS for sid, inner, n, K, chunk in SHAPES]


def _sources():
    return [os.path.join(EMU, "ndwt_emu_marchc.cpp"), os.path.join(EMU, "ndwt_emu.cpp")] + \
           [os.path.join(CSRC, h) for h in ("ndwt_device_axis.h", "ndwt_device.h", "ndwt_wave_row.h", "ndwt_geom.h", "ndwt_fused_tile.h",
                                            "ndwt_fused_list.h", "ndwt_taps_host.h")]


def _build(tag, flags, link_flags, out, extra=()):
    """ndwt_emu_marchc.cpp (and `extra` sources) compiled into tests/emu/build and linked to `out`; as make would, only what is older
    than its sources is rebuilt"""
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain is needed to build the host emulator")
    bdir = os.path.join(EMU, "build")
    os.makedirs(bdir, exist_ok=True)
    newest = max(os.path.getmtime(f) for f in _sources() + list(extra))
    objs = []
    for src in [_sources()[0]] + list(extra):
        obj = os.path.join(bdir, f"marchc_{tag}_{os.path.basename(src)}.o")
        if not os.path.exists(obj) or os.path.getmtime(obj) < newest:
            subprocess.check_call([CXX, "-std=c++17", "-fPIC", f"-I{CSRC}"] + flags + ["-c", src, "-o", obj])
        objs.append(obj)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(o) for o in objs):
        subprocess.check_call([CXX] + link_flags + objs + ["-o", out])
    return out


@pytest.fixture(scope="module")
def emu():
    so = _build("plain", ["-O1"], ["-shared", "-fPIC"], os.path.join(EMU, "libndwt_emu_marchc.so"))
    lib = ctypes.CDLL(so)
    lib.ndwt_emu_marchc.restype = ctypes.c_int
    lib.ndwt_emu_marchc.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 2 + [ctypes.c_longlong] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 2
    return lib


def _per_part(f, a):
    """the oracle on a complex array: the filters are real, so the transform of the real and of the imaginary part"""
    return f(a.real) + 1j * f(a.imag) if np.iscomplexobj(a) else f(a)


_MADE = {}


def make_case(cid, kind, wn, nlev, inner, n, K, inverse, l2=1):
    """(L, lo, hi, kernel-order input, oracle output [inner elements, n, K(, bands)], input in that shape, n): the input rounded to the
    kind's precision, the oracle in double on every (inner index, item) column on its own"""
    key = (cid, inverse)
    if key not in _MADE:
        rdt, cplx = KINDS[kind]
        comp = 2 if cplx else 1
        cdt = (np.complex64 if rdt == np.float32 else np.complex128) if cplx else rdt
        L = len(orc.wave_filters(wn)[0])
        n = L if n is None else n
        assert inner % comp == 0 and inner % 4 == 0 and n >= L
        ne = inner // comp                                    # elements of a sample
        rng = np.random.default_rng(zlib.crc32(repr((cid, inverse)).encode()))
        shape = (ne, n, K) + ((1 + nlev,) if inverse else ())
        a = rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if cplx else 0)
        a = a.astype(cdt).astype(np.complex128 if cplx else np.float64)
        one = (lambda v: orc.spatial_rec(v, [wn], l2)) if inverse else (lambda v: orc.spatial_dec(v, [wn], nlev, l2))
        want = np.zeros((ne, n, K) + (() if inverse else (1 + nlev,)), dtype=a.dtype)
        for c in range(ne):
            for k in range(K):
                want[c, :, k] = _per_part(one, a[c, :, k])
        t = kernel_taps(wn, l2)
        lo, hi = np.zeros(20), np.zeros(20)
        lo[:L], hi[:L] = (t["syn_lo"], t["syn_hi"]) if inverse else (t["ana_lo"], t["ana_hi"])
        _MADE[key] = (L, lo, hi, np.ascontiguousarray(to_kernel_order(a).astype(cdt)), want, a, n)
    return _MADE[key]


def _bound(kind, inverse, want, a):
    tol = TOL["single" if KINDS[kind][0] == np.float32 else "double"]
    return 2 * tol * max(np.abs(want).max(), np.abs(a).max()) if inverse else tol * np.abs(want).max()


def _cases(inverse):
    return [c for c in CASES if instantiated(inverse, KINDS[c[1]][0] == np.float64, len(orc.wave_filters(c[2])[0]), c[3])]


def test_the_case_list_is_what_the_table_leaves():
    """every case both ways, less the double 8-tap synthesis of 3 and 4 levels (the two instances that spill)"""
    assert len(_cases(False)) == len(CASES) == 64
    gone = [c[0] for c in CASES if c not in _cases(True)]
    assert len(gone) == 16 and all(("f64-db4" in g or "c128-db4" in g) for g in gone)


@pytest.mark.parametrize("inverse", [False, True], ids=["dec", "rec"])
@pytest.mark.parametrize("cid,kind,wn,nlev,inner,n,K,chunk", CASES, ids=[c[0] for c in CASES])
def test_emulated_cascaded_march(emu, cid, kind, wn, nlev, inner, n, K, chunk, inverse):
    rdt, cplx = KINDS[kind]
    L = len(orc.wave_filters(wn)[0])
    if not instantiated(inverse, rdt == np.float64, L, nlev):
        x = np.zeros(4 * L * (1 + nlev), dtype=rdt)            # not in the table: the emulator, which asks the table, refuses it
        assert emu.ndwt_emu_marchc(int(inverse), 1, L, nlev, x.ctypes.data, x.ctypes.data, 4, L, 1, 0, x.ctypes.data, x.ctypes.data) == -1
        return
    L, lo, hi, src, want, a, n = make_case(cid, kind, wn, nlev, inner, n, K, inverse)
    out = np.full(((K, n, src.shape[-1]) if inverse else (1 + nlev, K, n, src.shape[-1])), np.nan, dtype=src.dtype)
    rc = emu.ndwt_emu_marchc(int(inverse), int(rdt == np.float64), L, nlev, src.ctypes.data, out.ctypes.data, inner, n, K, chunk,
                             lo.ctypes.data, hi.ctypes.data)
    assert rc == 0
    got = np.transpose(out)
    assert np.isfinite(got).all()                             # every element of every band was written
    err, bound = np.abs(got - want).max(), _bound(kind, inverse, want, a)
    print(f"{cid} {'rec' if inverse else 'dec'}: {inner} scalars x {n} x {K}, chunk {chunk}: max error {err:.3g}, bound {bound:.3g}")
    assert err <= bound


def test_the_emulator_refuses_what_is_not_an_instance(emu):
    x = np.zeros(5 * 256, dtype=np.float32)
    t = np.zeros(20)
    for L, nlev, inner in ((10, 2, 8), (8, 5, 8), (8, 1, 8), (8, 2, 6), (8, 2, 2)):
        assert emu.ndwt_emu_marchc(0, 0, L, nlev, x.ctypes.data, x.ctypes.data, inner, 16, 1, 0, t.ctypes.data, t.ctypes.data) == -1


def test_the_cases_run_clean_under_address_and_ub_sanitizers(tmp_path):
    """the stand-alone program (its own main, -fsanitize=address,undefined) on every case above, as a child process"""
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    prog = _build("asan", san, ["-fsanitize=address,undefined"], os.path.join(EMU, "build", "ndwt_emu_marchc_asan"),
                  extra=[os.path.join(EMU, "ndwt_emu_marchc_main.cpp")])
    blob, ncases = [], 0
    for inverse in (False, True):
        for cid, kind, wn, nlev, inner, n, K, chunk in _cases(inverse):
            rdt, cplx = KINDS[kind]
            L, lo, hi, src, want, a, n = make_case(cid, kind, wn, nlev, inner, n, K, inverse)
            blob.append(struct.pack("<8i", int(inverse), int(rdt == np.float64), L, nlev, inner, n, K, chunk))
            blob.append(lo.astype("<f8").tobytes() + hi.astype("<f8").tobytes() + struct.pack("<d", float(_bound(kind, inverse, want, a))))
            blob.append(src.tobytes())
            blob.append(np.ascontiguousarray(to_kernel_order(want).astype(src.dtype)).tobytes())
            ncases += 1
    path = tmp_path / "cases.bin"
    path.write_bytes(struct.pack("<i", ncases) + b"".join(blob))
    r = subprocess.run([prog, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert f"{ncases} cases ok" in r.stdout
