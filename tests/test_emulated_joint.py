"""The joint-shrinkage kernels (JointShrink / GroupNorms of csrc/ndwt_device_joint.h, NormsFinish of csrc/ndwt_device_norms.h) emulated on
the host (tests/emu/ndwt_emu_joint.cpp: the kernel bodies compiled as plain C++, every thread of a workgroup run in turn between the
barriers) against numpy -- before any of it reaches a GPU.  Four kinds: float, complex64, double, complex128.

  shapes    5 items x 37 elements (the element-wise form, the group in registers, items off the 16- / 32-byte groups); 5 x 96 (the
            4-scalar form); 1, KREG and KREG + 1 items of 96 elements (one item: the group is the element; the last instance-wide unroll
            step; the first plan of two sweeps); 9 x 37 (two sweeps, element-wise); 40 x 96 (two sweeps, many turns of the load queue);
            2 x 20000 with the chunk count forced to 3 (a ragged last chunk; NormsFinish runs) and to 1
  array     3 bands on a pitch with guard scalars between and behind them.  Band 0: the contents of tests/norms_cases.py (random items,
            an all-equal item, an item with one NaN, an all-zero item with one -0, an integer-valued item); band 1 gets threshold 0 and
            must stay untouched; band 2 is integer-valued in every item
  values    the reference and the expectations of tests/joint_cases.py (derived there): the whole buffer bit for bit, soft and hard
  forms     the two-sweep form on a plan the registers form serves, and the element-wise form on an aligned array, give the same bytes:
            a group's arithmetic does not depend on who computes it
  norms     nnz and max exact, l1 and l2sq to the derived tolerance; a second run gives the same bits; the array is read only

The same cases run once more as a stand-alone program built with AddressSanitizer and UBSan (ndwt_emu_joint_main.cpp, the array a heap
block of exactly its size): a child process with nothing preloaded, which must exit 0.
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
KREG = 8                                                         # kJointReg (csrc/ndwt_select.h); test_kreg_is_the_librarys holds it

# (id, items, elements of one item, vec: 1 the 4-scalar form / 0 one element per step, guard scalars behind every band, chunks,
#  reg: 1 the group in registers / 0 two sweeps -- what the library's rule gives for that many items)
SHAPES = [
    ("5x37", 5, 37, 0, 3, 1, 1),
    ("5x96", 5, 96, 1, 4, 1, 1),
    ("1x96", 1, 96, 1, 4, 1, 1),
    (f"{KREG}x96", KREG, 96, 1, 4, 1, 1),
    (f"{KREG + 1}x96", KREG + 1, 96, 1, 4, 1, 0),
    ("9x37", 9, 37, 0, 3, 1, 0),
    ("40x96", 40, 96, 1, 4, 1, 0),
    ("2x20000-3chunks", 2, 20000, 1, 8, 3, 1),
    ("2x20000-1chunk", 2, 20000, 1, 8, 1, 1),
]
CASES = [(f"{kind}-{sid}", kind) + tuple(rest) for kind in KINDS for sid, *rest in SHAPES]


def _sources():
    return [os.path.join(EMU, "ndwt_emu_joint.cpp"), os.path.join(EMU, "ndwt_emu.cpp")] + \
           [os.path.join(CSRC, h) for h in ("ndwt_device_joint.h", "ndwt_device_norms.h", "ndwt_device_select.h", "ndwt_device.h", "ndwt_select.h",
                                            "ndwt_shrink.h", "ndwt_fused_list.h", "ndwt_geom.h", "ndwt_fused_tile.h", "ndwt_taps_host.h")]


def _build(tag, flags, link_flags, out, extra=()):
    """ndwt_emu_joint.cpp (and `extra` sources) compiled into tests/emu/build and linked to `out`; as make would, only what is older than
    its sources is rebuilt"""
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain is needed to build the host emulator")
    bdir = os.path.join(EMU, "build")
    os.makedirs(bdir, exist_ok=True)
    newest = max(os.path.getmtime(f) for f in _sources() + list(extra))
    objs = []
    for src in [_sources()[0]] + list(extra):
        obj = os.path.join(bdir, f"joint_{tag}_{os.path.basename(src)}.o")
        if not os.path.exists(obj) or os.path.getmtime(obj) < newest:
            subprocess.check_call([CXX, "-std=c++17", "-fPIC", f"-I{CSRC}"] + flags + ["-c", src, "-o", obj])
        objs.append(obj)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(o) for o in objs):
        subprocess.check_call([CXX] + link_flags + objs + ["-o", out])
    return out


@pytest.fixture(scope="module")
def emu():
    so = _build("plain", ["-O1"], ["-shared", "-fPIC"], os.path.join(EMU, "libndwt_emu_joint.so"))
    lib = ctypes.CDLL(so)
    lib.ndwt_emu_joint_shrink.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int,
                                                              ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    lib.ndwt_emu_group_norms.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int,
                                                             ctypes.c_int, ctypes.c_void_p]
    return lib


_MADE = {}


def make_case(cid, kind, items, N, guard):
    """(array, pitch, thresholds): made once per case and left unchanged"""
    if cid not in _MADE:
        src, pitch = joint_array(kind, items, N, NB, guard, zlib.crc32(cid.encode()) % 100000, integer_bands=(INT_BAND,))
        src.setflags(write=False)
        _MADE[cid] = (src, pitch, median_thresholds(kind, src, pitch, items, N, NB, zero_bands=(ZERO_BAND,)))
    return _MADE[cid]


def placed(data, vec, comp=1):
    """a copy at a 32-byte boundary (vec = 1), or one element past it (vec = 0: every block off the 16- / 32-byte groups of 4 scalars)"""
    raw = np.empty(data.nbytes + 64, dtype=np.uint8)
    off = (-raw.ctypes.data) % 32 + (0 if vec else comp * data.itemsize)
    out = raw[off:off + data.nbytes].view(data.dtype).reshape(data.shape)
    out[...] = data
    return out


def shrink(emu, kind, src, pitch, items, N, vec, reg, chunks, thr, hard, want=None):
    """the array after the emulated launch (a placed copy of src)"""
    rdt, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    y = placed(src, vec != 0, comp)
    t = np.ascontiguousarray(thr, dtype=np.float64)
    rc = emu.ndwt_emu_joint_shrink(int(rdt == np.float64), comp, vec, reg, y.ctypes.data, pitch, N * comp, items, NB, chunks, t.ctypes.data, int(hard))
    assert rc >= 0 and (want is None or rc == want), (rc, want)
    return y


def norms(emu, kind, y, pitch, items, N, vec, chunks):
    rdt, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    out = np.full((NB, 4), -1.0)
    rc = emu.ndwt_emu_group_norms(int(rdt == np.float64), comp, vec, y.ctypes.data, pitch, N * comp, items, NB, chunks, out.ctypes.data)
    assert rc == (vec if vec >= 0 else rc) and rc >= 0, rc
    return out


def test_kreg_is_the_librarys(emu):
    assert emu.ndwt_emu_joint_kreg() == KREG


@pytest.mark.parametrize("hard", [False, True], ids=["soft", "hard"])
@pytest.mark.parametrize("cid,kind,items,N,vec,guard,chunks,reg", CASES, ids=[c[0] for c in CASES])
def test_the_whole_buffer_after_the_shrink_against_numpy(emu, cid, kind, items, N, vec, guard, chunks, reg, hard):
    src, pitch, thr = make_case(cid, kind, items, N, guard)
    got = shrink(emu, kind, src, pitch, items, N, vec, reg, chunks, thr, hard, want=vec + 2 * reg)
    check_shrink(kind, src, got, pitch, items, N, NB, thr, hard, integer_bands=(INT_BAND,), what=cid)
    n = N * (2 if KINDS[kind][1] else 1)
    z = slice(ZERO_BAND * pitch, ZERO_BAND * pitch + items * n)
    assert got[z].tobytes() == src[z].tobytes()                    # (in check_shrink's comparison too; said once more: threshold 0)
    # what the library's rule decides for this placement and this many items is the form asked for
    assert shrink(emu, kind, src, pitch, items, N, -1 if vec else 0, -1, chunks, thr, hard, want=vec + 2 * reg).tobytes() == got.tobytes()
    # a group's arithmetic does not depend on the form: two sweeps where the registers serve, one element per step on an aligned array
    if reg:
        assert shrink(emu, kind, src, pitch, items, N, vec, 0, chunks, thr, hard, want=vec).tobytes() == got.tobytes()
    if vec:
        assert shrink(emu, kind, src, pitch, items, N, 0, reg, chunks, thr, hard, want=2 * reg).tobytes() == got.tobytes()


@pytest.mark.parametrize("cid,kind,items,N,vec,guard,chunks,reg", CASES, ids=[c[0] for c in CASES])
def test_the_group_norms_against_numpy(emu, cid, kind, items, N, vec, guard, chunks, reg):
    src, pitch, _ = make_case(cid, kind, items, N, guard)
    comp = 2 if KINDS[kind][1] else 1
    y = placed(src, vec != 0, comp)
    got = norms(emu, kind, y, pitch, items, N, vec, chunks)
    check_group_norms(kind, src, got, pitch, items, N, NB, integer_bands=(INT_BAND,), what=cid)
    assert y.tobytes() == src.tobytes()                            # the array is read only
    assert norms(emu, kind, y, pitch, items, N, vec, chunks).tobytes() == got.tobytes()   # the order of every sum is fixed: the same bits
    if vec:
        assert norms(emu, kind, y, pitch, items, N, -1, chunks).tobytes() == got.tobytes()
        other = norms(emu, kind, y, pitch, items, N, 0, chunks)   # (its sums are added in another order)
        assert np.array_equal(other[:, NNZ], got[:, NNZ]) and np.array_equal(other[:, MAX], got[:, MAX], equal_nan=True)
        check_group_norms(kind, src, other, pitch, items, N, NB, integer_bands=(INT_BAND,), what=cid + " element-wise")


def test_the_special_groups_are_what_the_case_says(emu):
    """five items: the group at position N // 2 of band 0 holds item 2's NaN and becomes zeros in every item, and it is the only NaN of
    the band, which therefore has NaN norms and counts that group; item 3 is zero with one -0, which keeps its sign where its group
    survives; hard mode leaves a surviving group's bits alone"""
    cid, kind, items, N, vec, guard, chunks, reg = [c for c in CASES if c[0] == "f32-5x96"][0]
    src, pitch, thr = make_case(cid, kind, items, N, guard)
    band0 = src[:items * N].reshape(items, N)
    assert np.isnan(band0).sum() == 1 and np.isnan(band0[2, N // 2])
    assert np.signbit(band0[3]).sum() == 1 and not band0[3].any()
    for hard in (False, True):
        got = shrink(emu, kind, src, pitch, items, N, vec, reg, chunks, thr, hard)[:items * N].reshape(items, N)
        assert not np.isnan(got).any()
        assert got[:, N // 2].tobytes() == np.zeros(items, dtype=src.dtype).tobytes()
        kept = got[0] != 0
        assert 0 < kept.sum() < N
        if hard:
            assert got[:, kept].tobytes() == band0[:, kept].tobytes()
        p = N // 3                                                # item 3's -0
        assert np.signbit(band0[3, p]) and (np.signbit(got[3, p]) == bool(kept[p]))
    v = norms(emu, kind, placed(src, 1), pitch, items, N, vec, chunks)
    for b in (0, ZERO_BAND):                                      # (the norms know no thresholds: band 1 has its NaN as well)
        assert np.isnan(v[b, [L1, L2SQ, MAX]]).all() and v[b, NNZ] == N
    assert not np.isnan(v[INT_BAND]).any()


def test_one_item_is_the_element(emu):
    """a plan of one real item: the group is the element, m = |c|, hard mode keeps c where |c| > t and stores +0 elsewhere"""
    cid, kind, items, N, vec, guard, chunks, reg = [c for c in CASES if c[0] == "f64-1x96"][0]
    src, pitch, thr = make_case(cid, kind, items, N, guard)
    got = shrink(emu, kind, src, pitch, items, N, vec, reg, chunks, thr, True)
    for b in (0, INT_BAND):
        c = src[b * pitch:b * pitch + N]
        assert got[b * pitch:b * pitch + N].tobytes() == np.where(np.abs(c) > thr[b], c, 0.0).tobytes()


def test_the_emulator_refuses_what_cannot_run(emu):
    y = placed(np.zeros(3 * 72, dtype=np.float32), 1)
    thr = np.ones(3)

    def call(comp, vec, pitch, n, items=2, chunks=1, reg=-1):
        return emu.ndwt_emu_joint_shrink(0, comp, vec, reg, y.ctypes.data, pitch, n, items, 3, chunks, thr.ctypes.data, 0)
    assert call(1, -1, 72, 32) == 3 and call(1, -1, 70, 32) == 2 and call(1, -1, 72, 30) == 2   # the rule: address, pitch, item length
    assert call(1, 1, 70, 32) == -1 and call(1, 1, 72, 30) == -1                                  # the 4-scalar form where it cannot run
    assert call(2, -1, 72, 31) == -1                                                              # half an element
    assert call(1, -1, 60, 32) == -1                                                              # a pitch smaller than a band
    assert call(1, -1, 72, 32, chunks=0) == -1
    assert call(1, -1, 72, 4, items=KREG + 1) == 1 and call(1, -1, 72, 4, items=KREG + 1, reg=1) == -1   # more items than registers


def test_the_cases_run_clean_under_address_and_ub_sanitizers(tmp_path):
    """the stand-alone program (its own main, -fsanitize=address,undefined) on every case above, soft and hard alternating, as a child
    process"""
    san = ["-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    prog = _build("asan", san, ["-fsanitize=address,undefined"], os.path.join(EMU, "build", "ndwt_emu_joint_asan"),
                  extra=[os.path.join(EMU, "ndwt_emu_joint_main.cpp")])
    blob = []
    for i, (cid, kind, items, N, vec, guard, chunks, reg) in enumerate(CASES):
        rdt, cplx = KINDS[kind]
        comp = 2 if cplx else 1
        n = N * comp
        hard = i % 2
        src, pitch, thr = make_case(cid, kind, items, N, guard)
        want = reference_norms(kind, src, pitch, items, N, NB, fused=True)
        tol = np.zeros((NB, 4))
        tol[:, L1] = N * 2.0 ** -52
        tol[:, L2SQ] = N * 2.0 ** -52
        tol[INT_BAND, L2SQ] = 0.0
        expect = reference_shrink(kind, src, pitch, items, N, NB, thr, hard, fused=True)
        total = (NB - 1) * pitch + items * n
        blob.append(struct.pack("<7i3q", int(rdt == np.float64), comp, vec, reg, chunks, NB, hard, n, items, pitch))
        blob.append(thr.astype("<f8").tobytes() + want.astype("<f8").tobytes() + tol.astype("<f8").tobytes())
        blob.append(src[:total].tobytes() + expect[:total].tobytes())
    path = tmp_path / "cases.bin"
    path.write_bytes(struct.pack("<i", len(CASES)) + b"".join(blob))
    r = subprocess.run([prog, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert f"{len(CASES)} cases ok" in r.stdout
