"""The per-item kernels (ItemSelect / ShrinkItems of csrc/ndwt_device_items.h) emulated on the host (tests/emu/ndwt_emu_select_items.cpp:
the kernel bodies compiled as plain C++, every thread of a workgroup run in turn between the barriers, the atomics plain adds) against
numpy -- before any of it reaches a GPU.  Four kinds: float, complex64, double, complex128.

  shapes    5 items x 37 elements (the element-wise form, items off the 16- / 32-byte groups, below one workgroup); 5 x 96 (the 4-scalar
            form); 3 x 4096 (several turns of the loop); 2 x 10000 (a ragged last turn); 1 item
  ranks     0, N - 1 and the two middle ranks in one call; one rank twice in one call -- N the elements of ONE item
  items     tests/items_cases.py: item j a draw of its own scaled by j + 1, item 1 all-equal, item 2 with a NaN
  real      bit for bit np.sort(|item j|)[k]; complex: the counting check of select_cases.check_complex, item by item
  contents  every content of tests/select_cases.py as the items of one call, on the 37- and the 4096-element items
  keys      the emulator checks that slot r of item j is one 64-bit word and that slots past nk are not written
  pick      BandPick -- its scan now pick_scan, shared with ItemSelect -- against the scan written out in numpy, on histograms with
            aliased and diverging slots (tests/test_emulated_select.py holds the whole band-wide select to numpy as before)
  shrink    ShrinkItems against shrink_group element by element: a zero entry leaves its block alone, the 4-scalar and element-wise forms

The same cases run once more as a stand-alone program built with AddressSanitizer and UBSan (ndwt_emu_select_items_main.cpp, the items a
heap block of exactly their size): a child process with nothing preloaded, which must exit 0.
"""
import ctypes
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from items_cases import check_items, item_ranks, items_band
from select_cases import COMPLEX_CONTENTS, KINDS, REAL_CONTENTS, complex_band, real_band

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "non-decimated_wavelets_amd", "csrc")
CXX = "/opt/rocm/lib/llvm/bin/clang++"

# (id, items, elements of one item, vec: 1 the 4-scalar form / 0 one element per step)
SHAPES = [
    ("5x37", 5, 37, 0),
    ("5x96", 5, 96, 1),
    ("3x4096", 3, 4096, 1),
    ("2x10000", 2, 10000, 1),
    ("1x96", 1, 96, 1),
]
CASES = [(f"{kind}-{sid}", kind, items, N, vec) for kind in KINDS for sid, items, N, vec in SHAPES]


def _sources():
    return [os.path.join(EMU, "ndwt_emu_select_items.cpp"), os.path.join(EMU, "ndwt_emu.cpp")] + \
           [os.path.join(CSRC, h) for h in ("ndwt_device_items.h", "ndwt_device_select.h", "ndwt_device.h", "ndwt_select.h", "ndwt_shrink.h",
                                            "ndwt_fused_list.h", "ndwt_geom.h", "ndwt_fused_tile.h", "ndwt_taps_host.h")]


def _build(tag, flags, link_flags, out, extra=()):
    """ndwt_emu_select_items.cpp (and `extra` sources) compiled into tests/emu/build and linked to `out`; as make would, only what is
    older than its sources is rebuilt"""
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain is needed to build the host emulator")
    bdir = os.path.join(EMU, "build")
    os.makedirs(bdir, exist_ok=True)
    newest = max(os.path.getmtime(f) for f in _sources() + list(extra))
    objs = []
    for src in [_sources()[0]] + list(extra):
        obj = os.path.join(bdir, f"items_{tag}_{os.path.basename(src)}.o")
        if not os.path.exists(obj) or os.path.getmtime(obj) < newest:
            subprocess.check_call([CXX, "-std=c++17", "-fPIC", f"-I{CSRC}"] + flags + ["-c", src, "-o", obj])
        objs.append(obj)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(o) for o in objs):
        subprocess.check_call([CXX] + link_flags + objs + ["-o", out])
    return out


@pytest.fixture(scope="module")
def emu():
    so = _build("plain", ["-O1"], ["-shared", "-fPIC"], os.path.join(EMU, "libndwt_emu_select_items.so"))
    lib = ctypes.CDLL(so)
    lib.ndwt_emu_select_items.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p,
                                          ctypes.c_void_p]
    lib.ndwt_emu_band_pick.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.ndwt_emu_shrink_items.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_void_p,
                                          ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    return lib


_MADE = {}


def make_items(cid, kind, items, N):
    if cid not in _MADE:
        _MADE[cid] = items_band(kind, items, N, zlib.crc32(cid.encode()))
    return _MADE[cid]


def placed(data, vec, comp=1):
    """a copy at a 32-byte boundary (vec = 1), or one element past it (vec = 0: every item off the 16- / 32-byte groups of 4 scalars)"""
    raw = np.empty(data.nbytes + 64, dtype=np.uint8)
    off = (-raw.ctypes.data) % 32 + (0 if vec else comp * data.itemsize)
    out = raw[off:off + data.nbytes].view(data.dtype).reshape(data.shape)
    out[...] = data
    return out


def run(emu, kind, y, ks, vec):
    rdt, cplx = KINDS[kind]
    k = np.asarray(ks, dtype=np.int64)
    out = np.full((y.shape[0], len(ks)), -1.0)
    rc = emu.ndwt_emu_select_items(int(rdt == np.float64), 2 if cplx else 1, vec, y.ctypes.data, y.shape[1], y.shape[0], len(ks), k.ctypes.data,
                                   out.ctypes.data)
    assert rc == 0, rc
    return out


@pytest.mark.parametrize("cid,kind,items,N,vec", CASES, ids=[c[0] for c in CASES])
def test_every_item_of_the_launch_against_numpy(emu, cid, kind, items, N, vec):
    src = make_items(cid, kind, items, N)
    y = placed(src, vec, 2 if KINDS[kind][1] else 1)
    for ks in item_ranks(N):
        check_items(kind, src, ks, run(emu, kind, y, ks, vec), cid)
    assert y.tobytes() == src.tobytes()                           # the items are read only
    if vec:                                                       # what select_vec decides for this placement is the form asked for
        assert run(emu, kind, y, item_ranks(N)[0], -1).tobytes() == run(emu, kind, y, item_ranks(N)[0], 1).tobytes()
        assert run(emu, kind, y, item_ranks(N)[0], 0).tobytes() == run(emu, kind, y, item_ranks(N)[0], 1).tobytes()   # ... and changes no value


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("N,vec", [(37, 0), (4096, 1)])
def test_every_content_as_the_items_of_one_call(emu, kind, N, vec):
    rdt, cplx = KINDS[kind]
    contents = COMPLEX_CONTENTS if cplx else REAL_CONTENTS
    src = np.stack([(complex_band if cplx else real_band)(rdt, N, c, 100 + j) for j, c in enumerate(contents)])
    y = placed(src, vec, 2 if cplx else 1)
    for ks in item_ranks(N):
        check_items(kind, src, ks, run(emu, kind, y, ks, vec), f"{kind}-{N}-contents")
    assert y.tobytes() == src.tobytes()


def test_the_emulator_refuses_what_the_library_refuses(emu):
    y = placed(np.zeros((2, 64), dtype=np.float32), 1)
    out = np.zeros(8)

    def call(comp, vec, n, ks):
        k = np.asarray(ks, dtype=np.int64)
        return emu.ndwt_emu_select_items(0, comp, vec, y.ctypes.data, n, 2, len(ks), k.ctypes.data, out.ctypes.data)
    assert call(1, -1, 64, [0, 63]) == 0
    assert call(1, -1, 64, [64]) == -1 and call(1, -1, 64, [-1]) == -1          # a rank outside [0, N) of ONE item
    assert call(2, -1, 64, [32]) == -1 and call(2, -1, 64, [31]) == 0            # N counts elements, not scalars
    assert call(1, -1, 64, [0] * 5) == -1 and call(1, -1, 64, []) == -1          # 1 .. 4 ranks
    assert call(1, 1, 62, [0]) == -1                                             # the 4-scalar form on items that are not whole groups


def _pick_reference(hist, prefix, rank, owner, k, nk, first, shift):
    """one pick step as ndwt_device_select.h describes it: per slot, the digit at which the cumulative count of its owner's histogram
    passes the slot's rank; the owners' histograms zeroed; the new owner the lowest slot with the same prefix"""
    hist, prefix, rank, owner = hist.copy(), prefix.copy(), rank.copy(), owner.copy()
    newp, newr = prefix.copy(), rank.copy()
    for r in range(nk):
        want = int(k[r]) if first else int(rank[r])
        cum = np.cumsum(hist[owner[r]].astype(np.int64))
        b = int(np.searchsorted(cum, want, side="right"))
        b = min(b, hist.shape[1] - 1)
        newp[r] = int(prefix[r]) | (b << shift)
        newr[r] = want - (int(cum[b - 1]) if b else 0)
    for r in range(nk):
        if owner[r] == r:
            hist[r] = 0
    for r in range(nk):
        prefix[r], rank[r] = newp[r], newr[r]
        owner[r] = min(q for q in range(r + 1) if newp[q] == newp[r])
    return hist, prefix, rank, owner


def test_band_pick_keeps_its_state_transitions(emu):
    """BandPick through pick_scan: first pass (ranks from the arguments, every slot an alias of slot 0), slots that diverge, slots that stay
    aliased, a rank in the last bin, nk = 1 .. 4; for both key widths"""
    rng = np.random.default_rng(5)
    for f64 in (0, 1):
        for trial in range(12):
            nk = 1 + trial % 4
            first = trial < 4
            hist = np.zeros((4, 2048), dtype=np.uint32)
            owner = np.zeros(4, dtype=np.int32)
            prefix = np.zeros(4, dtype=np.uint64)
            if not first:                                         # slots 0 / 1 aliased, 2 and 3 on their own where they exist
                owner[:] = [0, 0, 2, 3]
                prefix[:] = [5 << 40, 5 << 40, 6 << 40, 9 << 40] if f64 else [5 << 21, 5 << 21, 6 << 21, 9 << 21]
            for r in sorted(set(int(o) for o in owner[:nk])):
                bins = rng.choice(2048, size=[1, 3, 40, 2048][trial % 4], replace=False)
                hist[r, bins] = rng.integers(1, 50, bins.size)
                if trial % 3 == 0:
                    hist[r, 2047] += 7                            # counts in the last bin
            totals = [int(hist[owner[r]].sum()) for r in range(4)]
            k = np.array([rng.integers(0, max(totals[r], 1)) for r in range(4)], dtype=np.uint32)
            if trial % 3 == 0:
                k[0] = totals[0] - 1                              # the last rank: the last bin
            if nk >= 2 and trial % 2 == 0:
                k[1] = k[0]                                       # one rank twice: the slots stay aliased
            rank = np.zeros(4, dtype=np.uint32) if first else k.copy()
            sh = (53 if f64 else 21) if first else 10             # the first digit of the key, or one below every prefix bit set above
            want = _pick_reference(hist, prefix, rank, owner, k, nk, first, sh)
            st = np.zeros(64, dtype=np.uint8)
            st[:32] = prefix.view(np.uint8)
            st[32:48] = rank.view(np.uint8)
            st[48:64] = owner.view(np.uint8)
            h = hist.copy()
            assert emu.ndwt_emu_band_pick(f64, st.ctypes.data, h.ctypes.data, k.ctypes.data, nk, 0 if first else 1, sh) == 0
            got = (h, st[:32].view(np.uint64), st[32:48].view(np.uint32), st[48:64].view(np.int32))
            for name, g, w in zip(("histogram", "prefix", "rank", "owner"), got, want):
                assert np.array_equal(g[:nk] if name != "histogram" else g, w[:nk] if name != "histogram" else w), (f64, trial, name, g, w)


@pytest.mark.parametrize("kind", list(KINDS))
def test_shrink_items_is_shrink_group_on_every_block_with_its_own_threshold(emu, kind):
    rdt, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    for items, N, pitch_extra, chunks in ((3, 37, 0, 1), (3, 96, 0, 2), (2, 1000, 4, 3), (2, 1000, 1, 3)):
        nb, n = 3, N * comp
        pitch = items * n + pitch_extra
        rng = np.random.default_rng(N + pitch_extra)
        src = rng.standard_normal(nb * pitch).astype(rdt)
        thr = np.round(rng.random((items, nb)) * 4) / 4            # (quarters: exact in either precision)
        thr[0, 0] = 0.0
        thr[items - 1, 1] = 0.0
        for hard in (0, 1):
            y = placed(src, 1)
            vec = emu.ndwt_emu_shrink_items(int(rdt == np.float64), comp, y.ctypes.data, pitch, n, thr.ctypes.data, items, nb, chunks, hard)
            assert vec == int(pitch % 4 == 0 and n % 4 == 0), (items, N, pitch_extra, vec)
            for b in range(nb):
                assert y[b * pitch + items * n:(b + 1) * pitch].tobytes() == src[b * pitch + items * n:(b + 1) * pitch].tobytes()   # the padding of a pitch
                for j in range(items):
                    got = y[b * pitch + j * n:b * pitch + (j + 1) * n]
                    blk = src[b * pitch + j * n:b * pitch + (j + 1) * n]
                    t = rdt(thr[j, b])
                    if t == 0:
                        assert got.tobytes() == blk.tobytes(), (b, j)
                        continue
                    if not cplx:
                        m = np.abs(blk)
                        want = np.where(m > t, blk if hard else np.where(blk < 0, blk + t, blk - t), rdt(0)).astype(rdt)
                        assert got.tobytes() == want.tobytes(), (kind, b, j, hard)
                    else:
                        re, im = blk[0::2].astype(np.float64), blk[1::2].astype(np.float64)
                        m = np.hypot(re, im)
                        g = np.where(m > t, 1.0 if hard else (m - t) / np.where(m > 0, m, 1), 0.0)
                        near = np.abs(m - t) <= 8 * np.finfo(rdt).eps * m          # a magnitude at the threshold may round to either side
                        tol = 8 * np.finfo(rdt).eps * np.maximum(m, 1)
                        ok = (np.abs(got[0::2] - re * g) <= tol) & (np.abs(got[1::2] - im * g) <= tol)
                        assert (ok | near).all(), (kind, b, j, hard)


def test_the_cases_run_clean_under_address_and_ub_sanitizers(tmp_path):
    """the stand-alone program (its own main, -fsanitize=address,undefined) on every case above, as a child process"""
    san = ["-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    prog = _build("asan", san, ["-fsanitize=address,undefined"], os.path.join(EMU, "build", "ndwt_emu_select_items_asan"),
                  extra=[os.path.join(EMU, "ndwt_emu_select_items_main.cpp")])
    blob, ncases = [], 0
    for cid, kind, items, N, vec in CASES:
        rdt, cplx = KINDS[kind]
        src = make_items(cid, kind, items, N)
        for ks in item_ranks(N):
            k4 = (list(ks) + [0] * 4)[:4]
            want = np.zeros((items, 4))
            if not cplx:
                want[:, :len(ks)] = np.sort(np.abs(src), axis=1)[:, np.asarray(ks)].astype(np.float64)
            blob.append(struct.pack("<5i", int(rdt == np.float64), 2 if cplx else 1, vec, len(ks), int(not cplx)))
            blob.append(struct.pack("<qq4q", src.shape[1], items, *k4) + want.astype("<f8").tobytes())
            blob.append(src.tobytes())
            ncases += 1
    path = tmp_path / "cases.bin"
    path.write_bytes(struct.pack("<i", ncases) + b"".join(blob))
    r = subprocess.run([prog, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert f"{ncases} cases ok" in r.stdout
