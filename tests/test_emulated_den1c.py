"""The one-launch denoise of a batched 1-D plan (Den1C of csrc/ndwt_device_1d.h) emulated on the host (tests/emu/ndwt_emu_den1c.cpp: the
kernel body compiled as plain C++, every lane of a wave run in turn) against numpy: the oracle's dec, a numpy shrink per band, the
oracle's rec, signal by signal -- before any of it reaches a GPU.  Four kinds (float, complex64, double, complex128) x soft / hard.

The shapes: two segments whose second one is partial and wraps around the row (n comp = WX + 32); the shortest row allowed (n comp = 64
with db4 at 4 levels: a wave wraps it several times); five signals of one segment each, so that the last workgroup has idle waves; one
level (db1); four levels (db3).  Thresholds are 1.5 gains[b] (gains: the l2 norm of band b of the oracle's dec of a unit impulse) with
band 0 at 0; one case has every threshold 0 (output = input to the rec bound) and one thresholds band 0 too.  Output buffers are
pre-filled with NaN and must come back finite.  The bound is the rec bound of tests/test_gpu_parity.py, 2 TOL max(|want|, |c|).

Hard mode: a coefficient within rounding of its threshold may fall either side, which can hide or fake a failure.  So every band's
threshold is placed in the middle of the widest gap between consecutive sorted oracle |c| among the 40 order statistics around that
band's median, and the test asserts that the gap is at least 200 TOL max|c| -- a condition on the input, computed from the oracle alone.

The same cases run once more as a stand-alone program built with AddressSanitizer and UBSan (ndwt_emu_den1c_main.cpp, every buffer a
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
PARTS = range(5)                                              # EMU_D1_PART: 0 the entry point, 1 .. 4 the kinds


def tile_width(f64, ew, L, nlev):
    """Den1C::WX: the lanes valid after nlev analysis and nlev synthesis levels, in whole 128-byte lines"""
    GLa, GRa = ((L // 2 - 1) * ew + 3) // 4, ((L // 2) * ew + 3) // 4
    GLs, GRs = ((L // 2) * ew + 3) // 4, ((L // 2 - 1) * ew + 3) // 4
    lpl = 4 if f64 else 8
    return 4 * ((64 - nlev * (GLa + GRa + GLs + GRs)) // lpl * lpl)


# (id, wavelet, levels, signals, scalars per row or None = WX + 32 of the kind, thresholds: "details" | "zero" | "all")
SHAPES = [
    ("two-segments-db4-3", "db4", 3, 3, None, "details"),
    ("shortest-row-db4-4", "db4", 4, 2, 64, "details"),
    ("idle-waves-db2-2", "db2", 2, 5, 96, "details"),
    ("one-level-db1", "db1", 1, 2, None, "details"),
    ("four-levels-db3", "db3", 4, 2, None, "details"),
    ("all-zero-db4-3", "db4", 3, 3, None, "zero"),
    ("band0-too-db2-2", "db2", 2, 5, 96, "all"),
]
CASES = [(f"{kind}-{sid}", kind, wn, nlev, K, row, which) for kind in KINDS for sid, wn, nlev, K, row, which in SHAPES]


def _sources():
    return [os.path.join(EMU, "ndwt_emu_den1c.cpp"), os.path.join(EMU, "ndwt_emu.cpp"), os.path.join(CSRC, "ndwt_device_1d.h"),
            os.path.join(CSRC, "ndwt_device.h"), os.path.join(CSRC, "ndwt_wave_row.h"), os.path.join(CSRC, "ndwt_geom.h"), os.path.join(CSRC, "ndwt_fused_tile.h"),
            os.path.join(CSRC, "ndwt_taps_host.h"), os.path.join(CSRC, "ndwt_shrink.h")]


def _build(tag, flags, link_flags, out, extra=()):
    """the parts of ndwt_emu_den1c.cpp (and `extra` sources) compiled in parallel into tests/emu/build, linked to `out`; as make
    would, only what is older than its sources is rebuilt"""
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain is needed to build the host emulator")
    bdir = os.path.join(EMU, "build")
    os.makedirs(bdir, exist_ok=True)
    newest = max(os.path.getmtime(f) for f in _sources() + list(extra))
    jobs = [(os.path.join(bdir, f"den1c_{tag}_{p}.o"), [f"-DEMU_D1_PART={p}", _sources()[0]]) for p in PARTS]
    jobs += [(os.path.join(bdir, f"den1c_{tag}_{os.path.basename(e)}.o"), [e]) for e in extra]

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
    so = _build("plain", ["-O1"], ["-shared", "-fPIC"], os.path.join(EMU, "libndwt_emu_den1c.so"))
    lib = ctypes.CDLL(so)
    lib.ndwt_emu1_denoise.restype = ctypes.c_int
    lib.ndwt_emu1_denoise.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 2 + [ctypes.c_longlong] * 2 + [ctypes.c_void_p] * 2 + [ctypes.c_int]
    return lib


def _per_part(f, a):
    """the oracle on a complex array: the filters are real, so the transform of the real and of the imaginary part"""
    return f(a.real) + 1j * f(a.imag) if np.iscomplexobj(a) else f(a)


def np_shrink_bands(c, thr, hard):
    """band b of c[..., b] shrunk by thr[b] (complex: the magnitude); 0 leaves the band as it is"""
    out = c.copy()
    for b, t in enumerate(thr):
        if t == 0:
            continue
        cb = c[..., b]
        m = np.abs(cb)
        out[..., b] = cb * (np.where(m > t, 1.0, 0.0) if hard else np.where(m > t, (m - t) / np.where(m > 0, m, 1.0), 0.0))
    return out


def band_gains(n, wn, nlev, l2=1):
    e = np.zeros(n)
    e[0] = 1.0
    return np.sqrt((orc.spatial_dec(e, [wn], nlev, l2) ** 2).sum(axis=0))


def gap_thresholds(c, tol, which):
    """hard mode: per band the middle of the widest gap among the 40 order statistics of |c| around the median; the gap must be wide"""
    nb = c.shape[-1]
    thr = np.zeros(nb)
    for b in range(nb):
        if b == 0 and which != "all":
            continue
        m = np.sort(np.abs(c[..., b]).reshape(-1))
        mid = m.size // 2
        w = m[max(mid - 20, 0):mid + 20]
        gaps = np.diff(w)
        i = int(np.argmax(gaps))
        assert gaps[i] >= 200 * tol * m.max(), f"band {b}: widest gap {gaps[i]:.3g} < {200 * tol * m.max():.3g}: choose another seed"
        thr[b] = 0.5 * (w[i] + w[i + 1])
    return thr


_MADE = {}


def make_case(cid, kind, wn, nlev, K, row, which, hard, l2=1):
    """(L, taps[4][20], thr, kernel-order input, oracle output [n, K], bound, scalars per row): the input rounded to the kind's
    precision, the reference in double, signal by signal"""
    key = (cid, hard)
    if key not in _MADE:
        rdt, cplx = KINDS[kind]
        comp = 2 if cplx else 1
        cdt = (np.complex64 if rdt == np.float32 else np.complex128) if cplx else rdt
        tol = TOL["single" if rdt == np.float32 else "double"]
        L = len(orc.wave_filters(wn)[0])
        if row is None:
            row = tile_width(rdt == np.float64, comp, L, nlev) + 32
        assert row % 4 == 0 and row % comp == 0 and row >= 8 * L
        n = row // comp
        rng = np.random.default_rng(zlib.crc32(repr((cid, wn, nlev, K, row)).encode()))
        x = rng.standard_normal((n, K)) + (1j * rng.standard_normal((n, K)) if cplx else 0)
        x = x.astype(cdt).astype(np.complex128 if cplx else np.float64)
        c = np.stack([_per_part(lambda v: orc.spatial_dec(v, [wn], nlev, l2), x[:, k]) for k in range(K)], axis=1)     # [n, K, bands]
        if which == "zero":
            thr = np.zeros(1 + nlev)
        elif hard:
            thr = gap_thresholds(c, tol, which)
        else:
            thr = 1.5 * band_gains(n, wn, nlev, l2)
            if which != "all":
                thr[0] = 0.0
        cs = np_shrink_bands(c, thr, hard)
        want = np.stack([_per_part(lambda v: orc.spatial_rec(v, [wn], l2), cs[:, k]) for k in range(K)], axis=1)
        bound = 2 * tol * max(np.abs(want).max(), np.abs(cs).max())
        t = kernel_taps(wn, l2)
        taps = np.zeros((4, 20))
        for i, name in enumerate(("ana_lo", "ana_hi", "syn_lo", "syn_hi")):
            taps[i, :L] = t[name]
        _MADE[key] = (L, taps, thr, np.ascontiguousarray(to_kernel_order(x).astype(cdt)), want, bound, row)
    return _MADE[key]


@pytest.mark.parametrize("cid,kind,wn,nlev,K,row,which", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("hard", [False, True], ids=["soft", "hard"])
def test_emulated_denoise_of_the_kind(emu, cid, kind, wn, nlev, K, row, which, hard):
    rdt, cplx = KINDS[kind]
    L, taps, thr, src, want, bound, row = make_case(cid, kind, wn, nlev, K, row, which, hard)
    out = np.full(src.shape, np.nan, dtype=src.dtype)
    rc = emu.ndwt_emu1_denoise(int(rdt == np.float64), 2 if cplx else 1, L, nlev, src.ctypes.data, out.ctypes.data, row, K, taps.ctypes.data,
                               thr.ctypes.data, int(hard))
    assert rc == 0
    got = np.transpose(out)
    assert np.isfinite(got).all()                             # every element of every signal was written
    err = np.abs(got - want).max()
    print(f"{cid} {'hard' if hard else 'soft'}: row {row} scalars, thresholds {np.array2string(thr, precision=4)}, max error {err:.3g}, bound {bound:.3g}")
    assert err <= bound
    if which != "zero":
        assert np.abs(want - np.transpose(src)).max() > 100 * bound      # the thresholds did something: the result is not the input


def test_the_emulator_refuses_what_is_not_an_instance(emu):
    x = np.zeros(256, dtype=np.float32)
    y = np.zeros(256, dtype=np.float32)
    t = np.zeros(80)
    for L, nlev, row in ((10, 2, 256), (8, 5, 256), (8, 0, 256), (8, 2, 254)):
        assert emu.ndwt_emu1_denoise(0, 0, 1, L, nlev, x.ctypes.data, y.ctypes.data, row, 1, t.ctypes.data, t.ctypes.data, 0) == -1


def test_the_cases_run_clean_under_address_and_ub_sanitizers(tmp_path):
    """the stand-alone program (its own main, -fsanitize=address,undefined) on every case above, as a child process"""
    san = ["-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    prog = _build("asan", san, ["-fsanitize=address,undefined"], os.path.join(EMU, "build", "ndwt_emu_den1c_asan"),
                  extra=[os.path.join(EMU, "ndwt_emu_den1c_main.cpp")])
    blob, ncases = [], 0
    for cid, kind, wn, nlev, K, row, which in CASES:
        rdt, cplx = KINDS[kind]
        for hard in (False, True):
            L, taps, thr, src, want, bound, r = make_case(cid, kind, wn, nlev, K, row, which, hard)
            thr5 = np.zeros(5)
            thr5[:thr.size] = thr
            blob.append(struct.pack("<7i", int(rdt == np.float64), 2 if cplx else 1, L, nlev, r, K, int(hard)))
            blob.append(taps.astype("<f8").tobytes() + thr5.astype("<f8").tobytes() + struct.pack("<d", float(bound)))
            blob.append(src.tobytes())
            blob.append(np.ascontiguousarray(to_kernel_order(want).astype(src.dtype)).tobytes())
            ncases += 1
    path = tmp_path / "cases.bin"
    path.write_bytes(struct.pack("<i", ncases) + b"".join(blob))
    r = subprocess.run([prog, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert f"{ncases} cases ok" in r.stdout
