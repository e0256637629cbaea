"""The cascaded 2-D kernels (Fwd2C / Inv2C of csrc/ndwt_device.h) on a STACK of images, emulated on the host (tests/emu/ndwt_emu_stack2.cpp:
the kernel bodies compiled as plain C++, every lane of every wave of every item run in turn) against the numpy oracle applied to each item
alone -- before any of it reaches a GPU.

Four kinds x both directions.  Three items of n1 * comp = WX + 32 scalars (two tiles, the second anchored and wrapping around the row) by
40 rows; once with one chunk per item, once with chunks of 21 rows: two chunks per item, the second partial, and a march-in (21 rows for
db4 x 3 levels) that wraps inside the item -- a wave that read a neighbouring item's rows instead would miss the oracle.  db4 x 3 levels,
db2 x 2 levels, db1 x 3 levels.  Tolerances are those of tests/test_gpu_parity.py: 1e-12 (double), 2e-6 (single) relative for dec, and
2 TOL max(|want|, |c|) for rec.

The same cases run once more as a stand-alone program built with AddressSanitizer and UBSan (ndwt_emu_stack2_main.cpp, every buffer a
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
PARTS = range(9)                                              # EMU_STACK_PART: 0 the entry points, 1 .. 8 kind x direction
ITEMS, N2 = 3, 40
WAVELETS = [("db4", 3), ("db2", 2), ("db1", 3)]
CHUNKS = [0, 21]                                              # rows per wave: one chunk per item | two chunks, the second of 19 rows
CASES = [(f"{kind}-{wn}x{nlev}-{'one-chunk' if not yc else f'chunks-of-{yc}'}", kind, wn, nlev, yc)
         for kind in KINDS for wn, nlev in WAVELETS for yc in CHUNKS]


def _sources():
    return [os.path.join(EMU, "ndwt_emu_stack2.cpp"), os.path.join(EMU, "ndwt_emu.cpp"), os.path.join(CSRC, "ndwt_device.h"),
            os.path.join(CSRC, "ndwt_wave_row.h"), os.path.join(CSRC, "ndwt_geom.h"), os.path.join(CSRC, "ndwt_fused_tile.h"),
            os.path.join(CSRC, "ndwt_taps_host.h")]


def _build(tag, flags, link_flags, out, extra=()):
    """the parts of ndwt_emu_stack2.cpp (and `extra` sources) compiled in parallel into tests/emu/build, linked to `out`; as make would,
    only what is older than its sources is rebuilt"""
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain is needed to build the host emulator")
    bdir = os.path.join(EMU, "build")
    os.makedirs(bdir, exist_ok=True)
    newest = max(os.path.getmtime(f) for f in _sources() + list(extra))
    jobs = [(os.path.join(bdir, f"stack2_{tag}_{p}.o"), [f"-DEMU_STACK_PART={p}", _sources()[0]]) for p in PARTS]
    jobs += [(os.path.join(bdir, f"stack2_{tag}_{os.path.basename(e)}.o"), [e]) for e in extra]

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
    so = _build("plain", ["-O1"], ["-shared", "-fPIC"], os.path.join(EMU, "libndwt_emu_stack2.so"))
    lib = ctypes.CDLL(so)
    lib.ndwt_emu2_stack.restype = ctypes.c_int
    lib.ndwt_emu2_stack.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 2
    return lib


def _tile_width(inverse, f64, ew, L, nlev):
    """scalars of a row one wave stores: the lanes valid at every level, in whole 128-byte lines (csrc/ndwt_wave_row.h: WaveRowGeom)"""
    LH, RH = (L // 2, L // 2 - 1) if inverse else (L // 2 - 1, L // 2)
    GL, GR = (LH * ew + 3) // 4, (RH * ew + 3) // 4
    LPL = 32 // (8 if f64 else 4)
    return 4 * ((64 - nlev * (GL + GR)) // LPL * LPL)


def _taps(wn, l2, inverse):
    Lp = len(orc.wave_filters(wn)[0])
    lo, hi = np.zeros((3, 20)), np.zeros((3, 20))
    for ax in range(2):
        t = kernel_taps(wn, l2, Lp)
        lo[ax, :Lp], hi[ax, :Lp] = (t["syn_lo"], t["syn_hi"]) if inverse else (t["ana_lo"], t["ana_hi"])
    return Lp, lo, hi


def _per_part(f, a):
    """the oracle on a complex array: the filters are real, so the transform of the real and of the imaginary part"""
    return f(a.real) + 1j * f(a.imag) if np.iscomplexobj(a) else f(a)


_MADE = {}


def make_case(kind, wn, nlev, inverse, l2=1):
    """(Lp, lo, hi, n1 in scalars, kernel-order input, oracle output in MATLAB shape [n1, n2, items(, bands)], input in MATLAB shape): the
    input rounded to the kind's precision, the oracle -- item by item -- in double.  Made once per (kind, wavelet, direction)."""
    key = (kind, wn, nlev, inverse)
    if key not in _MADE:
        rdt, cplx = KINDS[kind]
        comp = 2 if cplx else 1
        cdt = (np.complex64 if rdt == np.float32 else np.complex128) if cplx else rdt
        Lp, lo, hi = _taps(wn, l2, inverse)
        n1s = _tile_width(inverse, rdt == np.float64, comp, Lp, nlev) + 32
        n1 = n1s // comp
        rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
        shape = (n1, N2, ITEMS) + ((1 + 3 * nlev,) if inverse else ())
        a = rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if cplx else 0)
        a = a.astype(cdt).astype(np.complex128 if cplx else np.float64)
        one = (lambda v: orc.spatial_rec(v, [wn, wn], l2)) if inverse else (lambda v: orc.spatial_dec(v, [wn, wn], nlev, l2))
        want = np.stack([_per_part(one, a[:, :, j]) for j in range(ITEMS)], axis=2)      # each item alone
        _MADE[key] = (Lp, lo, hi, n1s, np.ascontiguousarray(to_kernel_order(a).astype(cdt)), want, a)
    return _MADE[key]


def _bound(kind, inverse, want, a):
    tol = TOL["single" if KINDS[kind][0] == np.float32 else "double"]
    return 2 * tol * max(np.abs(want).max(), np.abs(a).max()) if inverse else tol * np.abs(want).max()


def test_the_shapes_are_two_tiles_of_the_kernels_own_width(emu):
    for kind, (rdt, cplx) in KINDS.items():
        for wn, nlev in WAVELETS:
            for inverse in (0, 1):
                Lp = len(orc.wave_filters(wn)[0])
                wx = emu.ndwt_emu2_stack_wx(inverse, int(rdt == np.float64), 2 if cplx else 1, Lp, nlev)
                assert wx > 0 and wx == _tile_width(inverse, rdt == np.float64, 2 if cplx else 1, Lp, nlev), (kind, wn, nlev, inverse, wx)
                assert make_case(kind, wn, nlev, bool(inverse))[3] == wx + 32


@pytest.mark.parametrize("cid,kind,wn,nlev,ychunk", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("inverse", [False, True], ids=["dec", "rec"])
def test_emulated_cascade_of_a_stack(emu, cid, kind, wn, nlev, ychunk, inverse):
    rdt, cplx = KINDS[kind]
    Lp, lo, hi, n1s, src, want, a = make_case(kind, wn, nlev, inverse)
    assert src.shape[-3:] == (ITEMS, N2, n1s // (2 if cplx else 1))
    out = np.full(((ITEMS, N2) if inverse else (1 + 3 * nlev, ITEMS, N2)) + src.shape[-1:], np.nan, dtype=src.dtype)
    rc = emu.ndwt_emu2_stack(int(inverse), int(rdt == np.float64), 2 if cplx else 1, Lp, nlev, src.ctypes.data, out.ctypes.data, n1s, N2, ITEMS, ychunk,
                             lo.ctypes.data, hi.ctypes.data)
    assert rc == 0
    got = np.transpose(out)
    assert np.isfinite(got).all()
    bound = _bound(kind, inverse, want, a)
    for j in range(ITEMS):
        err = np.abs(got[:, :, j] - want[:, :, j]).max()
        print(f"{cid} {'rec' if inverse else 'dec'} item {j}: max error {err:.3g}, bound {bound:.3g}")
        assert err <= bound, (cid, j)


@pytest.mark.parametrize("nbatch", [0, 1], ids=["zeroed-fields", "one-item"])
@pytest.mark.parametrize("inverse", [False, True], ids=["dec", "rec"])
def test_a_zeroed_batch_field_means_one_image(emu, nbatch, inverse):
    """nbatch = 0: the emulator leaves Fused2CArgs::nbatch and ::bstride as memset left them (what the sources that know nothing of
    stacks pass); nbatch = 1 with the stride of one image: what cascade2_launch passes for an unbatched plan.  Both are the single
    image's transform."""
    Lp, lo, hi, n1s, src, want, a = make_case("f32", "db2", 2, inverse)
    one = np.ascontiguousarray(src[:, 1] if inverse else src[1])
    out = np.full(((N2, n1s) if inverse else (7, N2, n1s)), np.nan, dtype=np.float32)
    assert emu.ndwt_emu2_stack(int(inverse), 0, 1, Lp, 2, one.ctypes.data, out.ctypes.data, n1s, N2, nbatch, 21, lo.ctypes.data, hi.ctypes.data) == 0
    assert np.abs(np.transpose(out) - want[:, :, 1]).max() <= _bound("f32", inverse, want, a)


def test_the_cases_run_clean_under_address_and_ub_sanitizers(tmp_path):
    """the stand-alone program (its own main, -fsanitize=address,undefined) on every case above, as a child process"""
    san = ["-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    prog = _build("asan", san, ["-fsanitize=address,undefined"], os.path.join(EMU, "build", "ndwt_emu_stack2_asan"),
                  extra=[os.path.join(EMU, "ndwt_emu_stack2_main.cpp")])
    blob, n = [], 0
    for cid, kind, wn, nlev, ychunk in CASES:
        rdt, cplx = KINDS[kind]
        for inverse in (False, True):
            Lp, lo, hi, n1s, src, want, a = make_case(kind, wn, nlev, inverse)
            blob.append(struct.pack("<9i", int(inverse), int(rdt == np.float64), 2 if cplx else 1, Lp, nlev, n1s, N2, ITEMS, ychunk))
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
