"""The band-norm kernels (BandNorms / NormsFinish of csrc/ndwt_device_norms.h) emulated on the host (tests/emu/ndwt_emu_norms.cpp: the
kernel bodies compiled as plain C++, every thread of a workgroup run in turn between the barriers) against numpy -- before any of it
reaches a GPU.  Four kinds: float, complex64, double, complex128.

  shapes    5 items x 37 elements (the element-wise form, items off the 16- / 32-byte groups, below one workgroup); 5 x 96 (the 4-scalar
            form); 2 x 20000 with the chunk count forced to 3 (a ragged last chunk; NormsFinish runs) and to 1; 1 item
  array     3 bands on a pitch with guard scalars between and behind them; the array is checked unchanged
  contents  tests/norms_cases.py: the items of tests/items_cases.py (an all-equal item; an item with one NaN -- only that item's l1 / l2sq
            / max are NaN, its nnz counts the NaN), an all-zero item with one -0, integer-valued items in [-8, 8]
  values    the reference and the tolerances of tests/norms_cases.py (derived there)
  order     the sums are a fixed function of the shape and the geometry: a second run gives the same bits; forcing the element-wise form
            on an aligned array changes no exact value

The same cases run once more as a stand-alone program built with AddressSanitizer and UBSan (ndwt_emu_norms_main.cpp, the array a heap
block of exactly its size): a child process with nothing preloaded, which must exit 0.
"""
import ctypes
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from norms_cases import L1, L2SQ, MAX, NNZ, check_array, norms_array, reference
from select_cases import KINDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "non-decimated_wavelets_amd", "csrc")
CXX = "/opt/rocm/lib/llvm/bin/clang++"
NB = 3

# (id, items, elements of one item, vec: 1 the 4-scalar form / 0 one element per step, guard scalars behind every band, chunks)
SHAPES = [
    ("5x37", 5, 37, 0, 3, 1),
    ("5x96", 5, 96, 1, 4, 1),
    ("2x20000-3chunks", 2, 20000, 1, 8, 3),
    ("2x20000-1chunk", 2, 20000, 1, 8, 1),
    ("1x96", 1, 96, 1, 4, 1),
]
CASES = [(f"{kind}-{sid}", kind, items, N, vec, guard, chunks) for kind in KINDS for sid, items, N, vec, guard, chunks in SHAPES]


def _sources():
    return [os.path.join(EMU, "ndwt_emu_norms.cpp"), os.path.join(EMU, "ndwt_emu.cpp")] + \
           [os.path.join(CSRC, h) for h in ("ndwt_device_norms.h", "ndwt_device_select.h", "ndwt_device.h", "ndwt_select.h", "ndwt_shrink.h",
                                            "ndwt_fused_list.h", "ndwt_geom.h", "ndwt_fused_tile.h", "ndwt_taps_host.h")]


def _build(tag, flags, link_flags, out, extra=()):
    """ndwt_emu_norms.cpp (and `extra` sources) compiled into tests/emu/build and linked to `out`; as make would, only what is older than
    its sources is rebuilt"""
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain is needed to build the host emulator")
    bdir = os.path.join(EMU, "build")
    os.makedirs(bdir, exist_ok=True)
    newest = max(os.path.getmtime(f) for f in _sources() + list(extra))
    objs = []
    for src in [_sources()[0]] + list(extra):
        obj = os.path.join(bdir, f"norms_{tag}_{os.path.basename(src)}.o")
        if not os.path.exists(obj) or os.path.getmtime(obj) < newest:
            subprocess.check_call([CXX, "-std=c++17", "-fPIC", f"-I{CSRC}"] + flags + ["-c", src, "-o", obj])
        objs.append(obj)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(o) for o in objs):
        subprocess.check_call([CXX] + link_flags + objs + ["-o", out])
    return out


@pytest.fixture(scope="module")
def emu():
    so = _build("plain", ["-O1"], ["-shared", "-fPIC"], os.path.join(EMU, "libndwt_emu_norms.so"))
    lib = ctypes.CDLL(so)
    lib.ndwt_emu_band_norms.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int,
                                                            ctypes.c_int, ctypes.c_void_p]
    return lib


_MADE = {}


def make_array(cid, kind, items, N, guard):
    if cid not in _MADE:
        _MADE[cid] = norms_array(kind, items, N, NB, guard, zlib.crc32(cid.encode()) % 100000)
    return _MADE[cid]


def placed(data, vec, comp=1):
    """a copy at a 32-byte boundary (vec = 1), or one element past it (vec = 0: every block off the 16- / 32-byte groups of 4 scalars)"""
    raw = np.empty(data.nbytes + 64, dtype=np.uint8)
    off = (-raw.ctypes.data) % 32 + (0 if vec else comp * data.itemsize)
    out = raw[off:off + data.nbytes].view(data.dtype).reshape(data.shape)
    out[...] = data
    return out


def run(emu, kind, y, pitch, items, N, vec, chunks):
    rdt, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    out = np.full((items, NB, 4), -1.0)
    rc = emu.ndwt_emu_band_norms(int(rdt == np.float64), comp, vec, y.ctypes.data, pitch, N * comp, items, NB, chunks, out.ctypes.data)
    assert rc == (vec if vec >= 0 else rc) and rc >= 0, rc
    return out


@pytest.mark.parametrize("cid,kind,items,N,vec,guard,chunks", CASES, ids=[c[0] for c in CASES])
def test_every_block_of_the_launch_against_numpy(emu, cid, kind, items, N, vec, guard, chunks):
    src, pitch, integer = make_array(cid, kind, items, N, guard)
    comp = 2 if KINDS[kind][1] else 1
    y = placed(src, vec, comp)
    got = run(emu, kind, y, pitch, items, N, vec, chunks)
    check_array(kind, src, pitch, items, N, NB, got, integer, cid)
    assert y.tobytes() == src.tobytes()                           # the array is read only
    assert run(emu, kind, y, pitch, items, N, vec, chunks).tobytes() == got.tobytes()   # the order of every sum is fixed: the same bits
    if vec:
        # what the library's rule decides for this placement is the form asked for ...
        assert run(emu, kind, y, pitch, items, N, -1, chunks).tobytes() == got.tobytes()
        # ... and the element-wise form on the same array changes no exact value (its sums are added in another order)
        other = run(emu, kind, y, pitch, items, N, 0, chunks)
        assert np.array_equal(other[..., NNZ], got[..., NNZ]) and np.array_equal(other[..., MAX], got[..., MAX], equal_nan=True)
        check_array(kind, src, pitch, items, N, NB, other, integer, cid + " element-wise")


def test_the_special_items_are_what_the_case_says(emu):
    """the contents are there: with five items, item 2 of every band holds its NaN and is the only NaN row, item 3 counts no non-zero
    (its -0 is zero), item 1 (all-equal) has max = l1 / N"""
    cid, kind, items, N, vec, guard, chunks = [c for c in CASES if c[0] == "f32-5x96"][0]
    src, pitch, _ = make_array(cid, kind, items, N, guard)
    got = run(emu, kind, placed(src, vec), pitch, items, N, vec, chunks)
    for b in range(NB):
        assert np.isnan(got[2, b, [L1, L2SQ, MAX]]).all() and got[2, b, NNZ] == N
        assert not np.isnan(np.delete(got[:, b], 2, axis=0)).any()
        assert got[3, b].tolist() == [0.0, 0.0, 0.0, 0.0]
        assert np.signbit(src[b * pitch + 3 * N:b * pitch + 4 * N]).sum() == 1
        assert got[1, b, MAX] * N == got[1, b, L1] and got[1, b, NNZ] == N


def test_the_emulator_refuses_what_cannot_run(emu):
    y = placed(np.zeros(3 * 72, dtype=np.float32), 1)
    out = np.zeros((2, 3, 4))

    def call(comp, vec, pitch, n, items=2, chunks=1):
        return emu.ndwt_emu_band_norms(0, comp, vec, y.ctypes.data, pitch, n, items, 3, chunks, out.ctypes.data)
    assert call(1, -1, 72, 32) == 1 and call(1, -1, 70, 32) == 0 and call(1, -1, 72, 30) == 0   # the rule: address, pitch, item length
    assert call(1, 1, 70, 32) == -1 and call(1, 1, 72, 30) == -1                                  # the 4-scalar form where it cannot run
    assert call(2, -1, 72, 31) == -1                                                              # half an element
    assert call(1, -1, 60, 32) == -1                                                              # a pitch smaller than a band
    assert call(1, -1, 72, 32, chunks=0) == -1


def test_the_cases_run_clean_under_address_and_ub_sanitizers(tmp_path):
    """the stand-alone program (its own main, -fsanitize=address,undefined) on every case above, as a child process"""
    san = ["-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    prog = _build("asan", san, ["-fsanitize=address,undefined"], os.path.join(EMU, "build", "ndwt_emu_norms_asan"),
                  extra=[os.path.join(EMU, "ndwt_emu_norms_main.cpp")])
    blob = []
    for cid, kind, items, N, vec, guard, chunks in CASES:
        rdt, cplx = KINDS[kind]
        comp = 2 if cplx else 1
        n = N * comp
        u = 2.0 ** -24 if rdt == np.float32 else 2.0 ** -53
        src, pitch, integer = make_array(cid, kind, items, N, guard)
        want, tol = np.zeros((items, NB, 4)), np.zeros((items, NB, 4))
        for b in range(NB):
            for j in range(items):
                blk = src[b * pitch + j * n:b * pitch + (j + 1) * n]
                with np.errstate(invalid="ignore"):
                    want[j, b] = reference(kind, blk)
                if np.isnan(blk).any():
                    want[j, b, :3] = np.nan
                exact = (b, j) in integer
                tol[j, b] = [(4 * u if cplx else 0.0) + (0.0 if exact and not cplx else n * 2.0 ** -52), 0.0 if exact else n * 2.0 ** -52,
                             4 * u if cplx else 0.0, 0.0]
        blob.append(struct.pack("<5i3q", int(rdt == np.float64), comp, vec, chunks, NB, n, items, pitch))
        blob.append(want.astype("<f8").tobytes() + tol.astype("<f8").tobytes())
        blob.append(src[:(NB - 1) * pitch + items * n].tobytes())
    path = tmp_path / "cases.bin"
    path.write_bytes(struct.pack("<i", len(CASES)) + b"".join(blob))
    r = subprocess.run([prog, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert f"{len(CASES)} cases ok" in r.stdout
