"""The SURE-statistics kernels (BandRisk / RiskFinish of csrc/ndwt_device_risk.h) emulated on the host (tests/emu/ndwt_emu_risk.cpp: the
kernel bodies compiled as plain C++, every thread of a workgroup run in turn between the barriers) against numpy -- before any of it
reaches a GPU.  Four kinds: float, complex64, double, complex128.

  shapes      those of tests/test_emulated_norms.py: 5 items x 37 elements (the element-wise form, items off the 16- / 32-byte groups,
              below one workgroup); 5 x 96 (the 4-scalar form); 2 x 20000 with the chunk count forced to 3 (a ragged last chunk;
              RiskFinish runs) and to 1; 1 item
  candidates  nc = 1, 3 and 8 (tests/risk_cases.py: a value of the data, +inf, 0, one below the smallest and one above the largest
              magnitude, ...), a row of its own for every block
  array       3 bands on a pitch with guard scalars between and behind them; the array is checked unchanged
  skipped     the blocks of band 1 begin their rows with a negative entry: zeros (and, the guard words being 1e30 and band 1's data
              like any other, a workgroup that read them would not return zeros)
  contents    tests/norms_cases.py: an all-equal item, an item with one NaN, an all-zero item with one -0, integer-valued items
  values      the reference and the tolerances of tests/risk_cases.py (derived there)
  order       the sums are a fixed function of the shape and the geometry: a second run gives the same bits

The same cases run once more as a stand-alone program built with AddressSanitizer and UBSan (ndwt_emu_risk_main.cpp, the array, the
candidates and the results heap blocks of exactly their sizes): a child process with nothing preloaded, which must exit 0.
"""
import ctypes
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from norms_cases import norms_array
from risk_cases import COUNT, ENERGY, INVSUM, blocks_of, candidate_row, check_block, reference
from select_cases import KINDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "non-decimated_wavelets_amd", "csrc")
CXX = "/opt/rocm/lib/llvm/bin/clang++"
NB = 3
SKIPPED_BAND = 1

# (id, items, elements of one item, vec: 1 the 4-scalar form / 0 one element per step, guard scalars behind every band, chunks)
SHAPES = [
    ("5x37", 5, 37, 0, 3, 1),
    ("5x96", 5, 96, 1, 4, 1),
    ("2x20000-3chunks", 2, 20000, 1, 8, 3),
    ("2x20000-1chunk", 2, 20000, 1, 8, 1),
    ("1x96", 1, 96, 1, 4, 1),
]
CASES = [(f"{kind}-{sid}-nc{nc}", kind, items, N, vec, guard, chunks, nc)
         for kind in KINDS for sid, items, N, vec, guard, chunks in SHAPES for nc in (1, 3, 8)]


def _sources():
    return [os.path.join(EMU, "ndwt_emu_risk.cpp"), os.path.join(EMU, "ndwt_emu.cpp")] + \
           [os.path.join(CSRC, h) for h in ("ndwt_device_risk.h", "ndwt_device_norms.h", "ndwt_device_select.h", "ndwt_device.h", "ndwt_select.h", "ndwt_shrink.h",
                                            "ndwt_fused_list.h", "ndwt_geom.h", "ndwt_fused_tile.h", "ndwt_taps_host.h")]


def _build(tag, flags, link_flags, out, extra=()):
    """ndwt_emu_risk.cpp (and `extra` sources) compiled into tests/emu/build and linked to `out`; as make would, only what is older than
    its sources is rebuilt"""
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain is needed to build the host emulator")
    bdir = os.path.join(EMU, "build")
    os.makedirs(bdir, exist_ok=True)
    newest = max(os.path.getmtime(f) for f in _sources() + list(extra))
    objs = []
    for src in [_sources()[0]] + list(extra):
        obj = os.path.join(bdir, f"risk_{tag}_{os.path.basename(src)}.o")
        if not os.path.exists(obj) or os.path.getmtime(obj) < newest:
            subprocess.check_call([CXX, "-std=c++17", "-fPIC", f"-I{CSRC}"] + flags + ["-c", src, "-o", obj])
        objs.append(obj)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(o) for o in objs):
        subprocess.check_call([CXX] + link_flags + objs + ["-o", out])
    return out


@pytest.fixture(scope="module")
def emu():
    so = _build("plain", ["-O1"], ["-shared", "-fPIC"], os.path.join(EMU, "libndwt_emu_risk.so"))
    lib = ctypes.CDLL(so)
    lib.ndwt_emu_band_risk.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int,
                                                           ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return lib


_MADE = {}


def make_case(cid, kind, items, N, vec, guard, nc):
    """(array, pitch, integer-valued blocks, candidates [items, NB, nc]) of a case, made once"""
    if cid not in _MADE:
        seed = zlib.crc32(cid.encode()) % 100000
        flat, pitch, integer = norms_array(kind, items, N, NB, guard, seed)
        cand = np.zeros((items, NB, nc))
        for b, j, blk in blocks_of(kind, flat, pitch, items, N, NB):
            cand[j, b] = candidate_row(kind, blk, nc, bool(vec), seed + 31 * b + j)
            if b == SKIPPED_BAND:
                cand[j, b, 0] = -1.0 - j
        _MADE[cid] = (flat, pitch, integer, cand)
    return _MADE[cid]


def placed(data, vec, comp=1):
    """a copy at a 32-byte boundary (vec = 1), or one element past it (vec = 0: every block off the 16- / 32-byte groups of 4 scalars)"""
    raw = np.empty(data.nbytes + 64, dtype=np.uint8)
    off = (-raw.ctypes.data) % 32 + (0 if vec else comp * data.itemsize)
    out = raw[off:off + data.nbytes].view(data.dtype).reshape(data.shape)
    out[...] = data
    return out


def run(emu, kind, y, pitch, items, N, vec, chunks, cand):
    rdt, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    cand = np.ascontiguousarray(cand, dtype=np.float64)
    nc = cand.shape[-1]
    out = np.full((items, NB, nc, 3), -1.0)
    rc = emu.ndwt_emu_band_risk(int(rdt == np.float64), comp, vec, y.ctypes.data, pitch, N * comp, items, NB, chunks, nc, cand.ctypes.data, out.ctypes.data)
    assert rc == (vec if vec >= 0 else rc) and rc >= 0, rc
    return out


def check_array(kind, flat, pitch, items, N, got, cand, vec, integer, what):
    for b, j, blk in blocks_of(kind, flat, pitch, items, N, NB):
        check_block(kind, blk, cand[j, b], got[j, b], bool(vec), (b, j) in integer, f"{what} band {b} item {j}")


@pytest.mark.parametrize("cid,kind,items,N,vec,guard,chunks,nc", CASES, ids=[c[0] for c in CASES])
def test_every_block_of_the_launch_against_numpy(emu, cid, kind, items, N, vec, guard, chunks, nc):
    src, pitch, integer, cand = make_case(cid, kind, items, N, vec, guard, nc)
    comp = 2 if KINDS[kind][1] else 1
    y = placed(src, vec, comp)
    got = run(emu, kind, y, pitch, items, N, vec, chunks, cand)
    check_array(kind, src, pitch, items, N, got, cand, vec, integer, cid)
    assert not got[:, SKIPPED_BAND].any()                         # the skipped band: zeros
    assert y.tobytes() == src.tobytes()                           # the array is read only
    assert run(emu, kind, y, pitch, items, N, vec, chunks, cand).tobytes() == got.tobytes()   # the order of every sum is fixed: the same bits
    if vec:
        # what the library's rule decides for this placement is the form asked for
        assert run(emu, kind, y, pitch, items, N, -1, chunks, cand).tobytes() == got.tobytes()
    if vec and not (kind == "c64"):
        # the element-wise form on the same array has the same magnitudes (all but complex64, whose two forms round differently): the
        # counts are the same, and its sums, added in another order, pass the same check
        other = run(emu, kind, y, pitch, items, N, 0, chunks, cand)
        assert np.array_equal(other[..., COUNT], got[..., COUNT])
        check_array(kind, src, pitch, items, N, other, cand, 1, integer, cid + " element-wise")


def test_the_special_items_are_what_the_case_says(emu):
    """with five items: item 2 of every band holds its NaN -- its energy is NaN at every candidate, at +inf its count is all N, and it is
    the only NaN row; item 3 (zeros, one -0) counts every element at t = 0 with energy 0; item 1 (all-equal) counts all N at its own
    magnitude and none below it"""
    kind, items, N = "f32", 5, 96
    src, pitch, _ = norms_array(kind, items, N, NB, 4, 11)
    cand = np.zeros((items, NB, 3))
    cand[:] = [0.0, np.inf, 1.0]
    eq = float(np.abs(src[N]))                                   # item 1 of band 0
    cand[1] = [eq, np.nextafter(np.float32(eq), np.float32(0)), 0.0]
    got = run(emu, kind, placed(src, 1), pitch, items, N, 1, 1, cand)
    for b in range(NB):
        assert np.isnan(got[2, b, :, ENERGY]).all() and got[2, b, 1, COUNT] == N and got[2, b, 0, COUNT] == 1
        assert not np.isnan(np.delete(got[:, b], 2, axis=0)).any()
        assert got[3, b, 0].tolist() == [N, 0.0, 0.0]
        assert got[1, b, :, COUNT].tolist() == [N, 0, 0] and got[1, b, 0, ENERGY] == N * eq * eq
        assert not got[..., INVSUM].any()


def test_the_emulator_refuses_what_cannot_run(emu):
    y = placed(np.zeros(3 * 72, dtype=np.float32), 1)
    out = np.zeros((2, 3, 8, 3))
    cand = np.zeros((2, 3, 8))

    def call(comp, vec, pitch, n, items=2, chunks=1, nc=8):
        return emu.ndwt_emu_band_risk(0, comp, vec, y.ctypes.data, pitch, n, items, 3, chunks, nc, cand.ctypes.data, out.ctypes.data)
    assert call(1, -1, 72, 32) == 1 and call(1, -1, 70, 32) == 0 and call(1, -1, 72, 30) == 0   # the rule: address, pitch, item length
    assert call(1, 1, 70, 32) == -1 and call(1, 1, 72, 30) == -1                                  # the 4-scalar form where it cannot run
    assert call(2, -1, 72, 31) == -1                                                              # half an element
    assert call(1, -1, 60, 32) == -1                                                              # a pitch smaller than a band
    assert call(1, -1, 72, 32, chunks=0) == -1
    assert call(1, -1, 72, 32, nc=0) == -1 and call(1, -1, 72, 32, nc=9) == -1


def test_the_cases_run_clean_under_address_and_ub_sanitizers(tmp_path):
    """the stand-alone program (its own main, -fsanitize=address,undefined) on every case above, as a child process"""
    san = ["-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    prog = _build("asan", san, ["-fsanitize=address,undefined"], os.path.join(EMU, "build", "ndwt_emu_risk_asan"),
                  extra=[os.path.join(EMU, "ndwt_emu_risk_main.cpp")])
    blob = []
    for cid, kind, items, N, vec, guard, chunks, nc in CASES:
        rdt, cplx = KINDS[kind]
        comp = 2 if cplx else 1
        n = N * comp
        src, pitch, integer, cand = make_case(cid, kind, items, N, vec, guard, nc)
        want, tol = np.zeros((items, NB, nc, 3)), np.zeros((items, NB, nc, 3))
        for b, j, blk in blocks_of(kind, src, pitch, items, N, NB):
            with np.errstate(invalid="ignore"):
                want[j, b] = reference(kind, blk, cand[j, b], bool(vec))
            if cand[j, b, 0] < 0:
                continue
            if np.isnan(blk).any():
                want[j, b, :, ENERGY] = np.nan
            tol[j, b, :, ENERGY] = 0.0 if (b, j) in integer else n * 2.0 ** -52
            tol[j, b, :, INVSUM] = n * 2.0 ** -52 if cplx else 0.0
        blob.append(struct.pack("<6i3q", int(rdt == np.float64), comp, vec, chunks, NB, nc, n, items, pitch))
        blob.append(cand.astype("<f8").tobytes() + want.astype("<f8").tobytes() + tol.astype("<f8").tobytes())
        blob.append(src[:(NB - 1) * pitch + items * n].tobytes())
    path = tmp_path / "cases.bin"
    path.write_bytes(struct.pack("<i", len(CASES)) + b"".join(blob))
    r = subprocess.run([prog, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert f"{len(CASES)} cases ok" in r.stdout
