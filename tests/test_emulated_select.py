"""The order statistics of a band (BandHist / BandPick of csrc/ndwt_device_select.h) emulated on the host (tests/emu/ndwt_emu_select.cpp:
the two kernel bodies compiled as plain C++, every thread of a workgroup run in turn between the barriers, the atomics plain adds,
the pass loop the library's) against numpy -- before any of it reaches a GPU.  Four kinds: float, complex64, double, complex128.

The cases are those of tests/test_gpu_select.py at their smallest (tests/select_cases.py holds the contents and the checks):
  bands   37 elements (below one workgroup, not a multiple of 4: one element per step); 4096 elements in the 4-scalar form and once
          more one element per step (what a band off its 16- / 32-byte alignment runs); 480 elements (a batch of 5 x 96); 10000
          elements on 3 workgroups of the 4-scalar form, so that every workgroup takes several turns of its loop with a ragged last one
  ranks   0, N - 1 and the two middle ranks in one call; one rank twice in one call
  real    every content on the 37- and the 4096-element band, Gaussian data on the others: values bit for bit those of numpy
  complex count(m < v (1 - eps)) <= k < count(m <= v (1 + eps)) with m = hypot(re, im) in double, eps = 4 machine epsilons
The emulator also checks that the pick step leaves the global histogram zero, and the band is compared with its copy afterwards.

The same cases run once more as a stand-alone program built with AddressSanitizer and UBSan (ndwt_emu_select_main.cpp, the band a
heap block of exactly its size): a child process with nothing preloaded, which must exit 0.
"""
import ctypes
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from select_cases import COMPLEX_CONTENTS, KINDS, REAL_CONTENTS, check_complex, check_real, complex_band, rank_sets, real_band

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "non-decimated_wavelets_amd", "csrc")
CXX = "/opt/rocm/lib/llvm/bin/clang++"

# (id, elements, vec: 1 the 4-scalar form / 0 one element per step, workgroups: 0 = what select_grid gives, contents: all or Gaussian only)
BANDS = [
    ("n37", 37, 0, 0, True),
    ("n4096-vec", 4096, 1, 0, True),
    ("n4096-elementwise", 4096, 0, 0, False),
    ("batch-5x96", 480, 1, 0, False),
    ("n10000-3-workgroups", 10000, 1, 3, False),
]
CASES = [(f"{kind}-{bid}-{content}", kind, N, vec, nblocks, content)
         for kind, (rdt, cplx) in KINDS.items() for bid, N, vec, nblocks, every in BANDS
         for content in ((COMPLEX_CONTENTS if cplx else REAL_CONTENTS) if every else ("gauss",))]


def _sources():
    return [os.path.join(EMU, "ndwt_emu_select.cpp"), os.path.join(EMU, "ndwt_emu.cpp"), os.path.join(CSRC, "ndwt_device_select.h"),
            os.path.join(CSRC, "ndwt_device.h"), os.path.join(CSRC, "ndwt_select.h"), os.path.join(CSRC, "ndwt_shrink.h"),
            os.path.join(CSRC, "ndwt_fused_list.h"), os.path.join(CSRC, "ndwt_geom.h"), os.path.join(CSRC, "ndwt_fused_tile.h"),
            os.path.join(CSRC, "ndwt_taps_host.h")]


def _build(tag, flags, link_flags, out, extra=()):
    """ndwt_emu_select.cpp (and `extra` sources) compiled into tests/emu/build and linked to `out`; as make would, only what is older
    than its sources is rebuilt"""
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain is needed to build the host emulator")
    bdir = os.path.join(EMU, "build")
    os.makedirs(bdir, exist_ok=True)
    newest = max(os.path.getmtime(f) for f in _sources() + list(extra))
    objs = []
    for src in [_sources()[0]] + list(extra):
        obj = os.path.join(bdir, f"select_{tag}_{os.path.basename(src)}.o")
        if not os.path.exists(obj) or os.path.getmtime(obj) < newest:
            subprocess.check_call([CXX, "-std=c++17", "-fPIC", f"-I{CSRC}"] + flags + ["-c", src, "-o", obj])
        objs.append(obj)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(o) for o in objs):
        subprocess.check_call([CXX] + link_flags + objs + ["-o", out])
    return out


@pytest.fixture(scope="module")
def emu():
    so = _build("plain", ["-O1"], ["-shared", "-fPIC"], os.path.join(EMU, "libndwt_emu_select.so"))
    lib = ctypes.CDLL(so)
    lib.ndwt_emu_select.restype = ctypes.c_int
    lib.ndwt_emu_select.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    return lib


_MADE = {}


def make_band(cid, kind, N, content):
    """the band of a case in kernel form (complex: interleaved scalars), made once"""
    if cid not in _MADE:
        rdt, cplx = KINDS[kind]
        seed = zlib.crc32(cid.encode())
        _MADE[cid] = complex_band(rdt, N, content, seed) if cplx else real_band(rdt, N, content, seed)
    return _MADE[cid]


def aligned_copy(y):
    """a copy at a 32-byte boundary (numpy promises 16): the 4-scalar form of double data needs it"""
    raw = np.empty(y.nbytes + 32, dtype=np.uint8)
    off = (-raw.ctypes.data) % 32
    out = raw[off:off + y.nbytes].view(y.dtype)
    out[:] = y
    return out


def run(emu, kind, y, ks, vec, nblocks):
    rdt, cplx = KINDS[kind]
    k = np.asarray(ks, dtype=np.int64)
    out = np.full(len(ks), -1.0)
    rc = emu.ndwt_emu_select(int(rdt == np.float64), 2 if cplx else 1, vec, y.ctypes.data, y.size, len(ks), k.ctypes.data, nblocks, out.ctypes.data)
    assert rc == 0
    return out


@pytest.mark.parametrize("cid,kind,N,vec,nblocks,content", CASES, ids=[c[0] for c in CASES])
def test_emulated_select_of_the_kind(emu, cid, kind, N, vec, nblocks, content):
    rdt, cplx = KINDS[kind]
    src = make_band(cid, kind, N, content)
    y = aligned_copy(src)
    for ks in rank_sets(N):
        got = run(emu, kind, y, ks, vec, nblocks)
        (check_complex if cplx else check_real)(src, ks, got, cid)
    assert y.tobytes() == src.tobytes()                           # the band is read only


def test_the_special_values_order_as_numpy_orders_them(emu):
    """zeros of both signs are one key, denormals lie between them and the normal values, the inf is the last number and the NaN the
    last order statistic -- rank by rank over the head and the tail of the band"""
    for kind in ("f32", "f64"):
        y = aligned_copy(real_band(KINDS[kind][0], 64, "special", 7))
        for ks in ([0, 1, 2, 3], [4, 5, 6, 7], [60, 61, 62, 63]):
            got = run(emu, kind, y, ks, 1, 0)
            check_real(y, ks, got, kind)
        tail = run(emu, kind, y, [62, 63], 1, 0)
        assert np.isinf(tail[0]) and np.isnan(tail[1])
        head = run(emu, kind, y, [0, 3, 4], 1, 0)
        assert head[0] == 0 and head[1] == 0 and not np.signbit(head[:2]).any() and 0 < head[2] < np.finfo(KINDS[kind][0]).tiny


def test_the_emulator_refuses_what_the_library_refuses(emu):
    y = aligned_copy(np.zeros(64, dtype=np.float32))
    out = np.zeros(4)

    def call(comp, vec, n, ks):
        k = np.asarray(ks, dtype=np.int64)
        return emu.ndwt_emu_select(0, comp, vec, y.ctypes.data, n, len(ks), k.ctypes.data, 0, out.ctypes.data)
    assert call(1, -1, 64, [0, 63]) == 0
    assert call(1, -1, 64, [64]) == -1 and call(1, -1, 64, [-1]) == -1          # a rank outside [0, N)
    assert call(2, -1, 64, [32]) == -1 and call(2, -1, 64, [31]) == 0            # N counts elements, not scalars
    assert call(1, -1, 64, [0] * 5) == -1 and call(1, -1, 64, []) == -1          # 1 .. 4 ranks
    assert call(3, -1, 63, [0]) == -1
    assert call(1, 1, 62, [0]) == -1                                             # the 4-scalar form on a band that is not whole groups


def test_the_cases_run_clean_under_address_and_ub_sanitizers(tmp_path):
    """the stand-alone program (its own main, -fsanitize=address,undefined) on every case above, as a child process"""
    san = ["-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    prog = _build("asan", san, ["-fsanitize=address,undefined"], os.path.join(EMU, "build", "ndwt_emu_select_asan"),
                  extra=[os.path.join(EMU, "ndwt_emu_select_main.cpp")])
    blob, ncases = [], 0
    for cid, kind, N, vec, nblocks, content in CASES:
        rdt, cplx = KINDS[kind]
        src = make_band(cid, kind, N, content)
        for ks in rank_sets(N):
            k4 = (list(ks) + [0] * 4)[:4]
            want = np.zeros(4)
            if not cplx:
                want[:len(ks)] = np.sort(np.abs(src))[np.asarray(ks)].astype(np.float64)
            blob.append(struct.pack("<6i", int(rdt == np.float64), 2 if cplx else 1, vec, len(ks), nblocks, int(not cplx)))
            blob.append(struct.pack("<q4q", src.size, *k4) + want.astype("<f8").tobytes())
            blob.append(src.tobytes())
            ncases += 1
    path = tmp_path / "cases.bin"
    path.write_bytes(struct.pack("<i", ncases) + b"".join(blob))
    r = subprocess.run([prog, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert f"{ncases} cases ok" in r.stdout
