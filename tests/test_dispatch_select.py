"""The dispatch pins of tests/test_gpu_dispatch.py, checked without a device: kernel selection is a function of integers
(csrc/ndwt_select.h), so every row whose level-1 launch is a fused 2-D / 3-D kernel is replayed against that header through a small
host shim (tests/select/select_shim.cpp, compiled with g++).  The GPU test reads what ran from the launch trace; this one asks the
same code what it would run."""
import ctypes
import os
import shutil
import subprocess

import pytest

import helpers
from test_gpu_dispatch import ROWS

HERE = os.path.dirname(os.path.abspath(__file__))
NUM_CUS = 256
# template parameters that follow from the tile table inside the kernel units: the pick does not carry them
NOT_IN_PICK = ("NT", "RY", "WLDS", "ZLDS")
# rows without a fused level-1 launch in either direction (1-D signals, the per-axis path on request, double with 18 taps)
LEFT_OUT = ["1d-vec4", "1d-ragged", "1d-c64", "1d-db7-plain", "generic-path", "f64-db9-per-axis"]
# LevelRouteKind of csrc/ndwt_select.h
FUSED3_DILATED, FUSED3, FUSED3_T, FUSED3_FOLD_T, FUSED2_DILATED, FUSED2, PER_AXIS = range(7)
WHOLE_ARRAY, SLAB_OUTER, SLAB_Z = range(3)                      # SlabMode


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++ to compile tests/select/select_shim.cpp")
    out = str(tmp_path_factory.mktemp("select") / "libselect_shim.so")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", os.path.join(HERE, "select", "select_shim.cpp"), "-o", out],
                   check=True)
    lib = ctypes.CDLL(out)
    lib.sel_fused3.restype = ctypes.c_char_p
    return lib


def _ints(v):
    return (ctypes.c_int * len(v))(*[int(x) for x in v])


def _plan(dims, lens, f64=False, cplx=False, generic=False, atrous=False, vf=0, vi=0):
    return _ints([len(dims), 2 if cplx else 1, f64, not cplx, not generic, atrous, 1] + (list(dims) + [1] * 4)[:4] + (list(lens) + [2] * 4)[:4] + [vf, vi])


def _route(shim, plan, stride, inverse, slab=WHOLE_ARRAY):
    Lp = ctypes.c_int(0)
    kind = shim.sel_level_path(plan, stride, 1 if inverse else 0, int(slab), ctypes.byref(Lp))
    return kind, Lp.value


def _route_dir(shim, plan, stride, direction, slab):
    Lp = ctypes.c_int(0)
    return shim.sel_level_path(plan, stride, int(direction), int(slab), ctypes.byref(Lp)), Lp.value


def _picks(shim, row, inverse):
    """the launches of the row's dec (rec) that kernel selection decides at tap stride 1, as (family, params)"""
    dims, d = row["dims"], len(row["dims"])
    wl = [row["wn"]] * d if isinstance(row["wn"], str) else row["wn"]
    lens = [2 * int(w[2:]) for w in wl]
    f64, comp = row["prec"] == "double", 2 if row["cplx"] else 1
    vf, vi = max(row["fwd"], 0), max(row["inv"], 0)
    plan = _plan(dims, lens, f64, row["cplx"], row["path"], row["dil"] == "atrous", vf, vi)
    n1 = dims[0] * comp
    vec4 = row["layout"] == "packed" and n1 % 4 == 0           # rows, band distances and pointers in whole groups of 4 scalars
    T = "double" if f64 else "float"
    (kind, L), out = _route(shim, plan, 1, inverse), []
    if kind in (FUSED3, FUSED3_T, FUSED3_FOLD_T):
        tfold = kind == FUSED3_FOLD_T and vec4                   # (the caller keeps the route for 16-byte-aligned pointers only)
        q = _ints([f64, inverse, vec4, wl[1] == wl[2], tfold, L] + lens[:3] + [comp, 1, n1, dims[1], dims[3] if d == 4 else 1, vf, vi, NUM_CUS, 0])
        r = (ctypes.c_int * 10)()
        name = shim.sel_fused3(q, r).decode()
        V, TX, TY, depth, scatter, uniyz, per_cu, target, pin, tpre = list(r)
        assert target == NUM_CUS * per_cu
        p = {"T": T, "L": L, "EW": comp, "TX": TX, "TY": TY, "VEC4": vec4}
        if name == "Fwd3":
            p.update(PIN=bool(pin), TPRE=bool(tpre))
        if name == "Inv3Y":
            p.update(XSC=bool(scatter), UNIYZ=bool(uniyz), DEPTH=depth)
        out.append((name, p))
    elif kind == FUSED2:
        left = row["level"]
        while True:                                              # the cascaded launches, then one launch per level
            n = shim.sel_cascade2_levels(plan, inverse, left)
            if n == 0:
                break
            p = {"T": T, "L": L, "NLEV": n}
            if inverse:
                p["PD"] = shim.sel_cascade2_rec_depth(vi)
            out.append(("Inv2C" if inverse else "Fwd2C", p))
            left -= n
        if left > 0:
            r = (ctypes.c_int * 4)()
            shim.sel_fused2(_ints([f64, inverse, vec4, L, comp, 1, n1, dims[1], vi]), r)
            if r[0] == 1:
                out.append(("Inv2P", {"T": T, "L": L, "PD": r[1], "PK": bool(r[2])}))
            else:
                out.append(("Inv2S" if inverse else "Fwd2S", {"T": T, "L": L, "EW": comp, "VEC4": vec4}))
    return out


def test_rows_pick_their_pinned_kernels(shim):
    checked = 0
    for prm in ROWS:
        row = prm.values[0]
        n = 0
        for inverse in (False, True):
            specs = [helpers.spec(s) for s in row["rec" if inverse else "dec"]]
            specs = [(fam, {k: v for k, v in p.items() if k not in NOT_IN_PICK}) for fam, p in specs]
            for fam, params in _picks(shim, row, inverse):
                rec = helpers._trace.KernelLaunch(fam, params)
                assert any(helpers.matches(rec, sp) for sp in specs), (prm.id, "rec" if inverse else "dec", rec, specs)
                n += 1
        assert (n == 0) == (prm.id in LEFT_OUT), (prm.id, n)
        checked += n > 0
    assert checked >= 73 and checked == len(ROWS) - len(LEFT_OUT)


# The route of a level on the whole array and on a slab, as the level functions and the slab entry points took it before level_route
# existed (written down from their if-chains, not from running it): (dims, wavelet orders x .. t, shard axis, stride, whole, slab), the
# same in both directions.  float real data; z-sharded plans 1 and 2 are plans of tests/test_gpu_zshard.py::test_mplan_z_slabs.
ROUTES = [
    ("3d-db4", [64, 64, 32], [4, 4, 4], 2, 1, FUSED3, FUSED3),
    ("3d-mixed-z-short", [64, 64, 32], [1, 3, 2], 2, 1, FUSED3, PER_AXIS),                 # the kernel would march 5 halo planes, the slab has 3
    ("4d-db4-on-t", [32, 32, 16, 16], [4, 4, 4, 4], 3, 1, FUSED3_T, FUSED3_T),              # t is the per-axis pass: any t filter
    ("4d-db4-on-t-t-longest", [32, 32, 16, 16], [2, 2, 2, 4], 3, 1, FUSED3_T, FUSED3_T),
    ("4d-db4-on-z", [24, 20, 24, 8], [4, 4, 4, 4], 2, 1, FUSED3_T, FUSED3_T),
    ("4d-mixed-z-short-on-z", [16, 12, 14, 5], [4, 2, 3, 2], 2, 1, FUSED3_T, PER_AXIS),
    ("4d-mixed-z-longest-on-z", [16, 12, 18, 5], [2, 3, 4, 2], 2, 1, FUSED3_T, FUSED3_T),
    ("2d-db4", [256, 256], [4, 4], 1, 1, FUSED2, FUSED2),
    ("2d-mixed-y-short", [256, 256], [4, 2], 1, 1, FUSED2, PER_AXIS),
    ("3d-atrous-stride2", [64, 64, 32], [4, 4, 4], 2, 2, FUSED3_DILATED, PER_AXIS),        # no sub-lattice form on slabs
    ("2d-atrous-stride2", [256, 256], [4, 4], 1, 2, FUSED2_DILATED, PER_AXIS),
    ("4d-atrous-stride2-on-z", [16, 12, 24, 4], [2, 2, 2, 2], 2, 2, PER_AXIS, PER_AXIS),
]


@pytest.mark.parametrize("name,dims,orders,shard,stride,whole,slab", ROUTES, ids=[r[0] for r in ROUTES])
def test_level_routes_whole_and_slab(shim, name, dims, orders, shard, stride, whole, slab):
    lens = [2 * k for k in orders]
    plan = _plan(dims, lens, atrous=stride > 1)
    Lp = max(lens[:3])
    for inverse in (False, True):
        assert _route(shim, plan, stride, inverse) == (whole, 0 if whole == PER_AXIS else Lp), (name, inverse)
        assert _route(shim, plan, stride, inverse, SLAB_OUTER if shard == len(dims) - 1 else SLAB_Z) == (slab, 0 if slab == PER_AXIS else Lp), (name, inverse)
    if len(dims) == 4 and shard == 2 and stride == 1:           # test_mplan_z_slabs: "scatter-add" in describe() for reference dilation
        assert (slab == FUSED3_T) == (lens[2] == max(lens[:3]))


def test_slab_rows_pick_their_pinned_kernels(shim):
    """the rows of tests/test_gpu_slab_dispatch.py, replayed the same way: level_route with the SlabMode of the row, then fused3_select /
    fused2_select with the local n1, n2 and the batch of every launch the slab entry points make (1; 2 in the _runs forms; the frames of a
    4-D volume) -- per cut and direction"""
    from test_gpu_slab_dispatch import ROWS as SLAB_ROWS
    fused = ("Fwd3", "Inv3", "Inv3S", "Inv3Y", "Fwd2S", "Inv2S", "Inv2P")
    checked = 0
    for prm in SLAB_ROWS:
        row = prm.values[0]
        dims, wl, ax, stride = row["dims"], row["wl"], row["axis"], row["stride"]
        d, lens = len(dims), [2 * int(w[2:]) for w in wl]
        f64, comp = row["prec"] == "double", 2 if row["cplx"] else 1
        T, n1 = "double" if f64 else "float", dims[0] * comp
        vec4 = n1 % 4 == 0 and (n1 * dims[1]) % 4 == 0
        mode = SLAB_OUTER if ax == d - 1 else SLAB_Z
        for z0, z1, _ in row["cuts"]:
            local = list(dims)
            local[ax] = z1 - z0
            plan = _plan(local, lens, f64, row["cplx"], False, stride > 1, max(row["fwd"], 0), max(row["inv"], 0))
            for inverse in (False, True):
                specs = [helpers.spec(s.lstrip("~")) for s in row["syn" if inverse else "ana"]]
                specs = [(fam, {k: v for k, v in p.items() if k not in NOT_IN_PICK}) for fam, p in specs]
                kind, L = _route(shim, plan, stride, inverse, mode)
                picks = []
                if kind in (FUSED3, FUSED3_T):
                    for nbatch in ([1, 2] if d == 3 else [local[3]] if ax == 2 else [local[3], local[3] + lens[3] - 1]):
                        q = _ints([f64, inverse, vec4, wl[1] == wl[2], 0, L] + lens[:3] + [comp, 1, n1, dims[1], nbatch, max(row["fwd"], 0),
                                  max(row["inv"], 0), NUM_CUS, 0])
                        r = (ctypes.c_int * 10)()
                        name = shim.sel_fused3(q, r).decode()
                        V, TX, TY, depth, scatter, uniyz, per_cu, target, pin, tpre = list(r)
                        p = {"T": T, "L": L, "EW": comp, "TX": TX, "TY": TY, "VEC4": vec4}
                        if name == "Fwd3":
                            p.update(PIN=bool(pin), TPRE=bool(tpre))
                        if name == "Inv3Y":
                            p.update(XSC=bool(scatter), UNIYZ=bool(uniyz), DEPTH=depth)
                        picks.append((name, p))
                elif kind == FUSED2:
                    r = (ctypes.c_int * 4)()
                    shim.sel_fused2(_ints([f64, inverse, vec4, L, comp, 1, n1, local[1], max(row["inv"], 0)]), r)
                    picks.append(("Inv2P", {"T": T, "L": L, "PD": r[1], "PK": bool(r[2])}) if r[0] == 1 else
                                 ("Inv2S" if inverse else "Fwd2S", {"T": T, "L": L, "EW": comp, "VEC4": vec4}))
                else:
                    assert kind == PER_AXIS and not any(fam in fused for fam, _ in specs), (prm.id, kind, specs)
                both, _ = _route_dir(shim, plan, 1, -1, mode)      # ndwt_plan_slab_fast: slab_fused3 for both directions at once, tap stride 1
                assert stride > 1 or row["fast"] == (both == FUSED3 or (both == FUSED3_T and mode == SLAB_Z)), (prm.id, both)
                for fam, params in picks:
                    rec = helpers._trace.KernelLaunch(fam, params)
                    assert any(helpers.matches(rec, sp) for sp in specs), (prm.id, (z0, z1), "syn" if inverse else "ana", rec, specs)
                    checked += 1
    assert checked >= 2 * 2 * 30
