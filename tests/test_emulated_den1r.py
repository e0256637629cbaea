"""Den1C with a threshold row per signal (Den1C<.., ROWTHR = true>, csrc/ndwt_device_1d.h) emulated on the host
(tests/emu/ndwt_emu_den1r.cpp) against its uniform twin, which tests/test_emulated_den1c.py holds to the oracle: the ROWTHR kernel on K
rows with a table, against Den1C<..> run K times with row j's uniform thresholds.  Row j must be BIT-IDENTICAL.

  K = 3: row 0 all-zero thresholds, row 1 all non-zero, row 2 zero for some bands; soft and hard
  float db4 at 4 levels, n = 416: 3 segments of WX = 192 with a ragged last one, so K nseg = 9 -- not a multiple of 4: the waves past
      the last item of the last workgroup are clamped onto it and must index inside the table
  float db1 at 1 level, n = 16; complex64 db2 at 3 levels; double db3 at 2 levels
The table is a heap block of exactly K x 5 scalars, and a.thr holds 1e30 in the ROWTHR run: a kernel that read it would zero everything.

The same cases run once more as a stand-alone program built with AddressSanitizer and UBSan (ndwt_emu_den1r_main.cpp): a child process
with nothing preloaded, which must exit 0.
"""
import ctypes
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from helpers import kernel_taps
from test_emulated_den1c import tile_width

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "non-decimated_wavelets_amd", "csrc")
CXX = "/opt/rocm/lib/llvm/bin/clang++"
K = 3
# (id, instance of the emulator, scalar type, scalars per element, wavelet, levels, elements of a row)
CASES = [
    ("f32-db4-4-n416", 0, np.float32, 1, "db4", 4, 416),
    ("f32-db1-1-n16", 1, np.float32, 1, "db1", 1, 16),
    ("c64-db2-3-n200", 2, np.float32, 2, "db2", 3, 200),
    ("f64-db3-2-n300", 3, np.float64, 1, "db3", 2, 300),
]


def _sources():
    return [os.path.join(EMU, "ndwt_emu_den1r.cpp"), os.path.join(EMU, "ndwt_emu.cpp")] + \
           [os.path.join(CSRC, h) for h in ("ndwt_device_1d.h", "ndwt_device.h", "ndwt_wave_row.h", "ndwt_geom.h", "ndwt_fused_tile.h", "ndwt_taps_host.h",
                                            "ndwt_shrink.h")]


def _build(tag, flags, link_flags, out, extra=()):
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain is needed to build the host emulator")
    bdir = os.path.join(EMU, "build")
    os.makedirs(bdir, exist_ok=True)
    newest = max(os.path.getmtime(f) for f in _sources() + list(extra))
    objs = []
    for src in [_sources()[0]] + list(extra):
        obj = os.path.join(bdir, f"den1r_{tag}_{os.path.basename(src)}.o")
        if not os.path.exists(obj) or os.path.getmtime(obj) < newest:
            subprocess.check_call([CXX, "-std=c++17", "-fPIC", f"-I{CSRC}"] + flags + ["-c", src, "-o", obj])
        objs.append(obj)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(o) for o in objs):
        subprocess.check_call([CXX] + link_flags + objs + ["-o", out])
    return out


@pytest.fixture(scope="module")
def emu():
    lib = ctypes.CDLL(_build("plain", ["-O1"], ["-shared", "-fPIC"], os.path.join(EMU, "libndwt_emu_den1r.so")))
    lib.ndwt_emu1r_denoise.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_int, ctypes.c_int]
    return lib


def make_case(cid, rdt, comp, wn, nlev, n):
    """(taps[4][20], thr[K][1 + nlev], the K rows in kernel form): row 0 all-zero thresholds, row 1 all non-zero, row 2 zero for some"""
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    x = rng.standard_normal((K, n * comp)).astype(rdt)
    thr = np.round(rng.random((K, 1 + nlev)) * 4 + 1) / 8          # eighths: exact in either precision
    thr[0] = 0.0
    thr[2, 0] = 0.0
    thr[2, nlev] = 0.0
    t = kernel_taps(wn, 1)
    taps = np.zeros((4, 20))
    for i, name in enumerate(("ana_lo", "ana_hi", "syn_lo", "syn_hi")):
        taps[i, :len(t[name])] = t[name]
    return taps, thr, x


def run(emu, which, x, taps, thr, hard, rowthr):
    out = np.full_like(x, np.nan)
    rc = emu.ndwt_emu1r_denoise(which, x.ctypes.data, out.ctypes.data, x.shape[1], x.shape[0], taps.ctypes.data, np.ascontiguousarray(thr).ctypes.data,
                                hard, rowthr)
    assert rc >= 0, rc
    return out, rc


@pytest.mark.parametrize("cid,which,rdt,comp,wn,nlev,n", CASES, ids=[c[0] for c in CASES])
def test_row_j_is_the_uniform_kernel_with_row_js_thresholds(emu, cid, which, rdt, comp, wn, nlev, n):
    taps, thr, x = make_case(cid, rdt, comp, wn, nlev, n)
    src = x.copy()
    for hard in (0, 1):
        got, tail = run(emu, which, x, taps, thr, hard, 1)
        assert not np.isnan(got).any()
        for j in range(K):
            one, _ = run(emu, which, x, taps, thr[j], hard, 0)
            assert got[j].tobytes() == one[j].tobytes(), (cid, hard, j)
        assert (got[0] != got[1]).any() and np.abs(got[0] - x[0]).max() <= 1e-4 * np.abs(x[0]).max() + 1e-5   # zero thresholds: the signal comes back
        if which == 0:                                            # 9 (row, segment) items: one wave in the last workgroup, three clamped
            nseg = -(-n // tile_width(False, 1, 8, 4))
            assert tile_width(False, 1, 8, 4) == 192 and nseg == 3 and tail == (K * nseg) % 4 == 1
    assert x.tobytes() == src.tobytes()


def test_the_cases_run_clean_under_address_and_ub_sanitizers(tmp_path):
    """the stand-alone program (its own main, -fsanitize=address,undefined) on every case above, as a child process"""
    san = ["-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    prog = _build("asan", san, ["-fsanitize=address,undefined"], os.path.join(EMU, "build", "ndwt_emu_den1r_asan"),
                  extra=[os.path.join(EMU, "ndwt_emu_den1r_main.cpp")])
    blob, ncases = [], 0
    for cid, which, rdt, comp, wn, nlev, n in CASES:
        taps, thr, x = make_case(cid, rdt, comp, wn, nlev, n)
        for hard in (0, 1):
            blob.append(struct.pack("<6i", which, int(rdt == np.float64), nlev, x.shape[1], K, hard))
            blob.append(taps.astype("<f8").tobytes() + thr.astype("<f8").tobytes() + x.tobytes())
            ncases += 1
    path = tmp_path / "cases.bin"
    path.write_bytes(struct.pack("<i", ncases) + b"".join(blob))
    r = subprocess.run([prog, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert f"{ncases} cases ok" in r.stdout
