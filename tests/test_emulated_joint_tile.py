"""The tile form of the joint-shrinkage kernels (JointTile / GroupNormsTile of csrc/ndwt_device_joint_tile.h) emulated on the host
(tests/emu/ndwt_emu_joint_tile.cpp: the kernel bodies compiled as plain C++, every thread of a workgroup run in turn between the barriers)
against the emulated chunk form (JointShrink / GroupNorms) and against numpy -- before any of it reaches a GPU.  Four kinds: float,
complex64, double, complex128; the 4-scalar form and the element-wise form of each.

SW (the steps of a strip) and J (the items of an LDS tile) are the kernels' own, read from the emulator library; a pass loads 256 / SW items.

  items     1, 256 / SW - 1 (one item short of a pass: rows that load nothing), J (the tile exactly), J + 1 (a second tile of one
            item), 3 J + 5 (more than three tiles, the last ragged)
  strips    2 SW + 1 steps (three strips, the last of one step) for every K; exactly SW steps (one strip: no NormsFinish) and, element-wise,
            SW - 1 (one ragged strip) for K = J + 1
  array     3 bands on a pitch with guard scalars between and behind them, the contents of tests/joint_cases.py: band 1 gets threshold
            0 and must stay untouched; band 2 is integer-valued in every item
  values    the whole buffer, guards included: bit for bit the emulated JointShrink's; against joint_cases.reference_shrink the float kinds
            bit for bit, the double kinds bit for bit against the fused reference and within DOUBLE_BOUND(K) of the plain loop
            (check_shrink); soft and hard
  norms     check_group_norms (nnz and max exact, l1 and l2sq to the derived tolerance); nnz and max are GroupNorms' bits; a second run
            gives the same bits; the array is read only

The same cases run once more as a stand-alone program built with AddressSanitizer and UBSan (ndwt_emu_joint_tile_main.cpp, the array a
heap block of exactly its size): a child process with nothing preloaded, which must exit 0.
"""
import ctypes
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from joint_cases import check_group_norms, check_shrink, joint_array, median_thresholds, reference_norms, reference_shrink
from norms_cases import L1, L2SQ, MAX, NNZ
from select_cases import KINDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "non-decimated_wavelets_amd", "csrc")
CXX = "/opt/rocm/lib/llvm/bin/clang++"
NB = 3
ZERO_BAND, INT_BAND = 1, 2

# the items of a case, from the kernels' J and the items of a pass
ITEMS = {"1": lambda J, rows: 1, "pass-1": lambda J, rows: rows - 1, "J": lambda J, rows: J, "J+1": lambda J, rows: J + 1, "3J+5": lambda J, rows: 3 * J + 5}
# the steps of a band, from the kernels' SW
STEPS = {"3strips": lambda SW: 2 * SW + 1, "1strip": lambda SW: SW, "1ragged": lambda SW: SW - 1}
# (id, kind, vec, items, steps)
CASES = [(f"{kind}-{'vec' if vec else 'elem'}-{k}-{st}", kind, vec, k, st)
         for kind in KINDS for vec in (1, 0)
         for k, st in [(k, "3strips") for k in ITEMS] + [("J+1", "1strip")] + ([] if vec else [("J+1", "1ragged")])]


def _sources():
    return [os.path.join(EMU, "ndwt_emu_joint_tile.cpp"), os.path.join(EMU, "ndwt_emu.cpp")] + \
           [os.path.join(CSRC, h) for h in ("ndwt_device_joint_tile.h", "ndwt_device_joint.h", "ndwt_device_norms.h", "ndwt_device_select.h", "ndwt_device.h",
                                            "ndwt_select.h", "ndwt_shrink.h", "ndwt_fused_list.h", "ndwt_geom.h", "ndwt_fused_tile.h", "ndwt_taps_host.h")]


def _build(tag, flags, link_flags, out, extra=()):
    """ndwt_emu_joint_tile.cpp (and `extra` sources) compiled into tests/emu/build and linked to `out`; as make would, only what is older
    than its sources is rebuilt"""
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain is needed to build the host emulator")
    bdir = os.path.join(EMU, "build")
    os.makedirs(bdir, exist_ok=True)
    newest = max(os.path.getmtime(f) for f in _sources() + list(extra))
    objs = []
    for src in [_sources()[0]] + list(extra):
        obj = os.path.join(bdir, f"jointtile_{tag}_{os.path.basename(src)}.o")
        if not os.path.exists(obj) or os.path.getmtime(obj) < newest:
            subprocess.check_call([CXX, "-std=c++17", "-fPIC", f"-I{CSRC}"] + flags + ["-c", src, "-o", obj])
        objs.append(obj)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(o) for o in objs):
        subprocess.check_call([CXX] + link_flags + objs + ["-o", out])
    return out


def _emu():
    so = _build("plain", ["-O1"], ["-shared", "-fPIC"], os.path.join(EMU, "libndwt_emu_joint_tile.so"))
    lib = ctypes.CDLL(so)
    lib.ndwt_emu_jt_shrink.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p,
                                                           ctypes.c_int]
    lib.ndwt_emu_jt_norms.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p]
    lib.ndwt_emu_jt_strips.argtypes = [ctypes.c_longlong, ctypes.c_int, ctypes.c_int]
    lib.ndwt_emu_jt_strips.restype = ctypes.c_longlong
    return lib


@pytest.fixture(scope="module")
def emu():
    return _emu()


_MADE = {}


def make_case(emu, cid, kind, vec, k, st):
    """(array, pitch, thresholds, items, elements of one item): made once per case and left unchanged"""
    if cid not in _MADE:
        SW, J = emu.ndwt_emu_jt_sw(), emu.ndwt_emu_jt_j()
        assert 256 % SW == 0 and J % (256 // SW) == 0
        comp = 2 if KINDS[kind][1] else 1
        items, steps = ITEMS[k](J, 256 // SW), STEPS[st](SW)
        N = steps * 4 // comp if vec else steps                   # the 4-scalar form: a step is 4 scalars; else one element
        guard = 4 if vec else 3
        src, pitch = joint_array(kind, items, N, NB, guard, zlib.crc32(cid.encode()) % 100000, integer_bands=(INT_BAND,))
        src.setflags(write=False)
        assert emu.ndwt_emu_jt_strips(N * comp, comp, vec) == {"3strips": 3, "1strip": 1, "1ragged": 1}[st]
        _MADE[cid] = (src, pitch, median_thresholds(kind, src, pitch, items, N, NB, zero_bands=(ZERO_BAND,)), items, N)
    return _MADE[cid]


def placed(data, vec, comp=1):
    """a copy at a 32-byte boundary (vec = 1), or one element past it (vec = 0: every block off the 16- / 32-byte groups of 4 scalars)"""
    raw = np.empty(data.nbytes + 64, dtype=np.uint8)
    off = (-raw.ctypes.data) % 32 + (0 if vec else comp * data.itemsize)
    out = raw[off:off + data.nbytes].view(data.dtype).reshape(data.shape)
    out[...] = data
    return out


def shrink(emu, kind, src, pitch, items, N, vec, tile, thr, hard):
    """the array after the emulated launch (a placed copy of src)"""
    rdt, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    y = placed(src, vec != 0, comp)
    t = np.ascontiguousarray(thr, dtype=np.float64)
    rc = emu.ndwt_emu_jt_shrink(int(rdt == np.float64), comp, vec, tile, y.ctypes.data, pitch, N * comp, items, NB, t.ctypes.data, int(hard))
    assert rc == vec, rc
    return y


def norms(emu, kind, y, pitch, items, N, vec, tile):
    rdt, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    out = np.full((NB, 4), -1.0)
    rc = emu.ndwt_emu_jt_norms(int(rdt == np.float64), comp, vec, tile, y.ctypes.data, pitch, N * comp, items, NB, out.ctypes.data)
    assert rc == vec, rc
    return out


def test_the_tile_is_whole_passes_and_fits_the_lds(emu):
    SW, J = emu.ndwt_emu_jt_sw(), emu.ndwt_emu_jt_j()
    assert SW >= 1 and 256 % SW == 0 and J % (256 // SW) == 0 and J >= 256 // SW
    assert J * SW * 32 + 256 * 32 <= 64 * 1024                    # complex128 / double in the 4-scalar form: 32 bytes a step, and the combine


@pytest.mark.parametrize("hard", [False, True], ids=["soft", "hard"])
@pytest.mark.parametrize("cid,kind,vec,k,st", CASES, ids=[c[0] for c in CASES])
def test_the_whole_buffer_against_the_chunk_form_and_numpy(emu, cid, kind, vec, k, st, hard):
    src, pitch, thr, items, N = make_case(emu, cid, kind, vec, k, st)
    got = shrink(emu, kind, src, pitch, items, N, vec, 1, thr, hard)
    old = shrink(emu, kind, src, pitch, items, N, vec, 0, thr, hard)
    assert got.tobytes() == old.tobytes()                          # JointShrink's bits, guards included
    check_shrink(kind, src, got, pitch, items, N, NB, thr, hard, integer_bands=(INT_BAND,), what=cid)
    n = N * (2 if KINDS[kind][1] else 1)
    z = slice(ZERO_BAND * pitch, ZERO_BAND * pitch + items * n)
    assert got[z].tobytes() == src[z].tobytes()                    # (in check_shrink's comparison too; said once more: threshold 0)
    assert not np.array_equal(got[:items * n], src[:items * n], equal_nan=True)   # (and band 0 was shrunk)


@pytest.mark.parametrize("cid,kind,vec,k,st", CASES, ids=[c[0] for c in CASES])
def test_the_group_norms_against_the_chunk_form_and_numpy(emu, cid, kind, vec, k, st):
    src, pitch, _, items, N = make_case(emu, cid, kind, vec, k, st)
    comp = 2 if KINDS[kind][1] else 1
    y = placed(src, vec != 0, comp)
    got = norms(emu, kind, y, pitch, items, N, vec, 1)
    check_group_norms(kind, src, got, pitch, items, N, NB, integer_bands=(INT_BAND,), what=cid)
    assert y.tobytes() == src.tobytes()                            # the array is read only
    assert norms(emu, kind, y, pitch, items, N, vec, 1).tobytes() == got.tobytes()   # the order of every sum is fixed: the same bits
    old = norms(emu, kind, y, pitch, items, N, vec, 0)            # every group's s and m are the chunk form's bits
    assert old[:, NNZ].tobytes() == got[:, NNZ].tobytes() and old[:, MAX].tobytes() == got[:, MAX].tobytes()


def test_the_cases_run_clean_under_address_and_ub_sanitizers(emu, tmp_path):
    """the stand-alone program (its own main, -fsanitize=address,undefined) on every case above, soft and hard alternating, as a child
    process"""
    san = ["-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    prog = _build("asan", san, ["-fsanitize=address,undefined"], os.path.join(EMU, "build", "ndwt_emu_joint_tile_asan"),
                  extra=[os.path.join(EMU, "ndwt_emu_joint_tile_main.cpp")])
    blob = []
    for i, (cid, kind, vec, k, st) in enumerate(CASES):
        rdt, cplx = KINDS[kind]
        comp = 2 if cplx else 1
        hard = i % 2
        src, pitch, thr, items, N = make_case(emu, cid, kind, vec, k, st)
        n = N * comp
        want = reference_norms(kind, src, pitch, items, N, NB, fused=True)
        tol = np.zeros((NB, 4))
        tol[:, L1] = N * 2.0 ** -52
        tol[:, L2SQ] = N * 2.0 ** -52
        tol[INT_BAND, L2SQ] = 0.0
        expect = reference_shrink(kind, src, pitch, items, N, NB, thr, hard, fused=True)
        total = (NB - 1) * pitch + items * n
        blob.append(struct.pack("<5i3q", int(rdt == np.float64), comp, vec, NB, hard, n, items, pitch))
        blob.append(thr.astype("<f8").tobytes() + want.astype("<f8").tobytes() + tol.astype("<f8").tobytes())
        blob.append(src[:total].tobytes() + expect[:total].tobytes())
    path = tmp_path / "cases.bin"
    path.write_bytes(struct.pack("<i", len(CASES)) + b"".join(blob))
    r = subprocess.run([prog, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert f"{len(CASES)} cases ok" in r.stdout
