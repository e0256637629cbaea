"""The neighbourhood-shrinkage kernel (NeighShrink<T, COMP, ND, R> of csrc/ndwt_device_neigh.h) emulated on the host
(tests/emu/ndwt_emu_neigh.cpp: the kernel body compiled as plain C++, every thread of a workgroup run in turn between the barriers) against
numpy -- before any of it reaches a GPU.  All 36 instances: float, complex64, double, complex128 x 1, 2, 3 filtered axes x radius 1, 2, 3.

The cases run as a stand-alone program built with AddressSanitizer and UBSan (ndwt_emu_neigh_main.cpp; the input and the output heap blocks
of exactly their sizes): a child process with nothing preloaded, which must exit 0.  The program compares the whole output, the scalars
between the bands included, bit for bit with neigh_cases.reference_neigh computed with the exact fma (for the float kinds that is plain
numpy), and the input with what it was.

Shapes (neigh_cases.shape_list, from the tile of the instance under test, tests/select/neigh_shim.cpp):
  window        every filtered axis exactly 2r + 1 long: every neighbour wraps; the thresholds just below the median of S
  tile+1  axes of TX + 1 (TY + 1), the marched axis 3 (2r + 1) + 2 long with the smallest chunk: three chunks, every seam and the
                wrap of the ring's priming
  2tile-1       axes of 2 TX - 1 (2 TY - 1): two tiles, the second one short of full
  items         3 items: a window must not leak into the neighbouring item
  constant      3 constant items a_j = j + 1, hard, t^2 = 6 M between M a_1^2 and M a_2^2: items 0 and 1 all zero, item 2 untouched
every instance runs `window`; the other shapes run for every kind and number of axes with the radius rotating.  The array is that of
neigh_cases.neigh_array (an integer-valued band, a NaN, an all-zero item, -0, guards of 1e30), at a pitch with guard scalars; band
ZERO_BAND gets threshold 0 in the shapes with 3 items and must arrive as a copy.
"""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from neigh_cases import (BIG, INT_BAND, OUT_FILL, ZERO_BAND, geometry, levels_for, median_thresholds, neigh_array, neigh_shim, num_bands, pack_case, reference_neigh, shape_list)
from select_cases import KINDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "non-decimated_wavelets_amd", "csrc")
CXX = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return neigh_shim(tmp_path_factory)


def _sources():
    return [os.path.join(EMU, "ndwt_emu_neigh.cpp"), os.path.join(EMU, "ndwt_emu_neigh_main.cpp"), os.path.join(EMU, "ndwt_emu.cpp")] + \
           [os.path.join(CSRC, h) for h in ("ndwt_device_neigh.h", "ndwt_device_joint.h", "ndwt_device_norms.h", "ndwt_device_select.h", "ndwt_device.h",
                                            "ndwt_select.h", "ndwt_shrink.h", "ndwt_fused_list.h", "ndwt_geom.h", "ndwt_fused_tile.h", "ndwt_taps_host.h")]


def _build_program():
    """ndwt_emu_neigh.cpp and its main compiled with the sanitizers into tests/emu/build; as make would, only what is older than its
    sources is rebuilt"""
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain is needed to build the host emulator")
    bdir = os.path.join(EMU, "build")
    os.makedirs(bdir, exist_ok=True)
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    newest = max(os.path.getmtime(f) for f in _sources())
    objs = []
    for src in _sources()[:2]:
        obj = os.path.join(bdir, f"neigh_asan_{os.path.basename(src)}.o")
        if not os.path.exists(obj) or os.path.getmtime(obj) < newest:
            subprocess.check_call([CXX, "-std=c++17", "-fPIC", f"-I{CSRC}"] + san + ["-c", src, "-o", obj])
        objs.append(obj)
    out = os.path.join(bdir, "ndwt_emu_neigh_asan")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(o) for o in objs):
        subprocess.check_call([CXX, "-fsanitize=address,undefined"] + objs + ["-o", out])
    return out


def cases(shim):
    """[(id, kind, nd, r, shape id, dims, items, hard)]"""
    out = []
    for ki, (kind, (rdt, cplx)) in enumerate(KINDS.items()):
        eb = np.dtype(rdt).itemsize * (2 if cplx else 1)
        for nd in (1, 2, 3):
            for r in (1, 2, 3):
                for sid, dims, items in shape_list(nd, r, shim.sel_neigh_tx(nd), shim.sel_neigh_ty(nd, eb, r)):
                    if sid != "window" and r != 1 + (ki + nd) % 3:   # (the radius rotates over the kinds and the numbers of axes)
                        continue
                    out.append((f"{kind}-{nd}d-r{r}-{sid}", kind, nd, r, sid, dims, items, len(out) % 2))
    return out


def build_case(shim, cid, kind, nd, r, sid, dims, items, hard):
    rdt, cplx = KINDS[kind]
    nb = num_bands(nd, levels_for(nd))
    src, lead, pitch = neigh_array(kind, items, dims, nb, 3, zlib.crc32(cid.encode()) % 100000)
    thr = median_thresholds(kind, src, lead, pitch, items, dims, nb, r, zero_bands=(ZERO_BAND,) if items > 1 else (), below=sid == "window")
    geom = geometry(shim, nd, dims, np.dtype(rdt).itemsize * (2 if cplx else 1), r, nb * items, 256, BIG)
    expect = reference_neigh(kind, src, lead, pitch, items, dims, nb, thr, r, hard, fused=True)
    return pack_case(kind, nd, r, hard, dims, items, lead, pitch, nb, geom, thr, src, expect), geom, thr, src, expect, lead, pitch, nb


def constant_case(shim, kind, nd, r):
    """3 constant items 1, 2, 3 in every band, hard, t^2 = 6 M"""
    rdt, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    w = 2 * r + 1
    dims = [w + 2, w + 1, w][:nd]
    nb = num_bands(nd, levels_for(nd))
    n = int(np.prod(dims)) * comp
    pitch, lead, items = 3 * n + 5, 5, 3
    src = np.full(lead + nb * pitch, 1e30, dtype=rdt)
    for b in range(nb):
        for j in range(items):
            blk = src[lead + b * pitch + j * n:lead + b * pitch + (j + 1) * n]
            blk[...] = 0
            blk[::comp] = j + 1                                   # (complex: a_j + 0i)
    M = w ** nd
    thr = np.full(nb, float(np.sqrt(6.0 * M)))
    expect = np.full(src.shape, OUT_FILL, dtype=rdt)
    for b in range(nb):
        expect[lead + b * pitch:lead + b * pitch + 2 * n] = 0
        expect[lead + b * pitch + 2 * n:lead + b * pitch + 3 * n] = src[lead + b * pitch + 2 * n:lead + b * pitch + 3 * n]
    assert expect.tobytes() == reference_neigh(kind, src, lead, pitch, items, dims, nb, thr, r, True, fused=True).tobytes()
    geom = geometry(shim, nd, dims, np.dtype(rdt).itemsize * comp, r, nb * items, 256, BIG)
    return pack_case(kind, nd, r, True, dims, items, lead, pitch, nb, geom, thr, src, expect)


def test_the_reference_is_what_the_definition_says_on_a_hand_computed_case():
    """1-D, r = 1, float: x = 1 2 3 4 periodic; S = 21 14 29 26; t = 4, tt = 16: positions 0, 2, 3 survive"""
    src = np.array([1, 2, 3, 4], dtype=np.float32)
    got = reference_neigh("f32", src, 0, 4, 1, [4], 1, [4.0], 1, False)
    S = np.array([16 + 1 + 4, 1 + 4 + 9, 4 + 9 + 16, 9 + 16 + 1], dtype=np.float64)
    want = np.where(S > 16, src * ((S - 16) / S).astype(np.float32), np.float32(0)).astype(np.float32)
    assert got.tobytes() == want.tobytes() and got[1] == 0 and got[0] == np.float32(1 * np.float32(5 / 21))
    assert reference_neigh("f32", src, 0, 4, 1, [4], 1, [4.0], 1, True).tolist() == [1, 0, 3, 4]
    assert reference_neigh("f32", src, 0, 4, 1, [4], 1, [0.0], 1, False).tobytes() == src.tobytes()
    # 2-D, r = 1 on 3 x 3: every window is the whole item; complex: re and im both count
    z = np.arange(18, dtype=np.float64)
    S2 = float((z * z).sum())
    got = reference_neigh("c128", z, 0, 18, 1, [3, 3], 1, [1.0], 1, False, fused=True)
    assert np.array_equal(got, z * ((S2 - 1.0) / S2))


def test_every_instance_runs_clean_under_address_and_ub_sanitizers_and_matches_numpy(shim, tmp_path):
    prog = _build_program()
    blob, ids = [], []
    for c in cases(shim):
        packed, geom, thr, src, expect, lead, pitch, nb = build_case(shim, *c)
        cid, kind, nd, r, sid, dims, items, hard = c
        if sid == "tile+1" and nd >= 2:
            assert geom[3] == 3 and 2 * r + 1 <= geom[2] <= 2 * r + 2, (cid, geom)   # three chunks of the smallest size
        if items > 1:                                             # the zero-threshold band arrives as a copy, NaN and -0 included
            z = slice(lead + ZERO_BAND * pitch, lead + (ZERO_BAND + 1) * pitch - 3)
            assert thr[ZERO_BAND] == 0 and expect[z].tobytes() == src[z].tobytes()
        assert thr[INT_BAND] > 0
        blob.append(packed)
        ids.append(cid)
    for kind in KINDS:
        for nd in (1, 2, 3):
            blob.append(constant_case(shim, kind, nd, 1 + nd % 3))
            ids.append(f"{kind}-{nd}d-constant")
    seen = {(c[1], c[2], c[3]) for c in cases(shim)}
    assert len(seen) == 36                                        # every instance
    path = tmp_path / "cases.bin"
    path.write_bytes(struct.pack("<i", len(blob)) + b"".join(blob))
    r = subprocess.run([prog, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (ids[r.stdout.count("  ok:")] if r.stdout.count("  ok:") < len(ids) else "", r.stdout[-4000:])
    assert f"{len(blob)} cases ok" in r.stdout
