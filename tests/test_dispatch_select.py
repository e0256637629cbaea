"""The dispatch pins of tests/test_gpu_dispatch.py, checked without a device: kernel selection is a function of integers
(csrc/ndwt_select.h), so every row whose level-1 launch is a fused 2-D / 3-D kernel is replayed against that header through a small
host shim (tests/select/select_shim.cpp, compiled with g++).  The GPU test reads what ran from the launch trace; this one asks the
same code what it would run.  Every pick -- 3-D, one-level 2-D, Inv2P -- is an instance's full name, so every template parameter a row
pins (WPE of Fwd2S / Inv2S included) is compared, and every pick is looked up in the instance lists (csrc/ndwt_fused_list.h).  The
per-axis passes are picked the same way (axis_select): their tests are at the end of this file."""
import ctypes
import shutil

import pytest

import helpers
from test_gpu_dispatch import ROWS

NUM_CUS = 256
# template parameters of a pinned kernel that the pick does not name: none -- the pick is the instance's full name
NOT_IN_PICK = ()
# rows without a fused level-1 launch in either direction (1-D signals, the per-axis path on request, double with 18 taps, complex128
# images with 10)
LEFT_OUT = ["1d-vec4", "1d-ragged", "1d-c64", "1d-db7-plain", "generic-path", "f64-db9-per-axis", "2d-c128-db5-per-axis"]
# LevelRouteKind of csrc/ndwt_select.h
FUSED3_DILATED, FUSED3, FUSED3_T, FUSED3_FOLD_T, FUSED2_DILATED, FUSED2, PER_AXIS = range(7)
WHOLE_ARRAY, SLAB_OUTER, SLAB_Z = range(3)                      # SlabMode


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++ to compile tests/select/select_shim.cpp")
    return helpers.build_select_shim(str(tmp_path_factory.mktemp("select")))


def _fused3(shim, q):
    """fused3_select for the query: (kernel name, the trace parameters of the instance it names, the raw answer by field)"""
    r = (ctypes.c_int * 20)()
    name = shim.sel_fused3(_ints(q), r).decode()
    f = dict(zip(("V", "TX", "TY", "NT", "RY", "WPE", "PIN", "TPRE", "WLDS", "DEPTH", "ZLDS", "UNIYZ", "XSC", "per_cu", "target", "VEC4", "EW",
                  "L", "f64", "listed"), r))
    p = {"T": "double" if f["f64"] else "float", "L": f["L"], "EW": f["EW"], "TX": f["TX"], "TY": f["TY"], "NT": f["NT"], "WPE": f["WPE"],
         "VEC4": bool(f["VEC4"])}
    if name == "Fwd3":
        p.update(RY=f["RY"], PIN=bool(f["PIN"]), TPRE=bool(f["TPRE"]), WLDS=f["WLDS"], LOWONLY=False)
    if name in ("Inv3", "Inv3S"):
        p.update(RY=f["RY"])
    if name == "Inv3Y":
        p.update(XSC=bool(f["XSC"]), UNIYZ=bool(f["UNIYZ"]), DEPTH=f["DEPTH"], ZLDS=f["ZLDS"])
    return name, p, f


def _ints(v):
    return (ctypes.c_int * len(v))(*[int(x) for x in v])


def _fused2(shim, q):
    """fused2_select for the query [f64, inverse, vec4, Lp, ew, dil, n1, n2, variant_inv]: (kernel name, the trace parameters of the
    instance it names, the raw answer by field)"""
    r = (ctypes.c_int * 10)()
    shim.sel_fused2(_ints(q), r)
    f = dict(zip(("family", "inverse", "f64", "VEC4", "L", "EW", "WPE_or_PD", "PK", "waves", "listed"), r))
    assert (bool(f["f64"]), bool(f["inverse"]), f["L"]) == (bool(q[0]), bool(q[1]), q[3]), (q, f)
    T = "double" if f["f64"] else "float"
    if f["family"] == 1:
        assert f["inverse"] and f["VEC4"] and f["EW"] == 1, (q, f)
        return "Inv2P", {"T": T, "L": f["L"], "PD": f["WPE_or_PD"], "PK": bool(f["PK"])}, f
    assert (bool(f["VEC4"]), f["EW"]) == (bool(q[2]), q[4]), (q, f)
    return "Inv2S" if f["inverse"] else "Fwd2S", {"T": T, "L": f["L"], "VEC4": bool(f["VEC4"]), "WPE": f["WPE_or_PD"], "EW": f["EW"]}, f


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
        name, p, f = _fused3(shim, [f64, inverse, vec4, wl[1] == wl[2], tfold, L] + lens[:3] + [comp, 1, n1, dims[1], dims[3] if d == 4 else 1, vf, vi,
                                    NUM_CUS, 0])
        assert f["target"] == NUM_CUS * f["per_cu"] and (f["L"], f["EW"], bool(f["VEC4"]), bool(f["f64"])) == (L, comp, vec4, f64)
        assert f["listed"], (row, name, p)
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
            name, p, f = _fused2(shim, [f64, inverse, vec4, L, comp, 1, n1, dims[1], vi])
            assert f["listed"], (row, name, p)
            out.append((name, p))
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
                        name, p, f = _fused3(shim, [f64, inverse, vec4, wl[1] == wl[2], 0, L] + lens[:3] + [comp, 1, n1, dims[1], nbatch,
                                                    max(row["fwd"], 0), max(row["inv"], 0), NUM_CUS, 0])
                        assert f["listed"], (prm.id, name, p)
                        picks.append((name, p))
                elif kind == FUSED2:
                    name, p, f = _fused2(shim, [f64, inverse, vec4, L, comp, 1, n1, local[1], max(row["inv"], 0)])
                    assert f["listed"], (prm.id, name, p)
                    picks.append((name, p))
                else:
                    assert kind == PER_AXIS and not any(fam in fused for fam, _ in specs), (prm.id, kind, specs)
                both, _ = _route_dir(shim, plan, 1, -1, mode)      # ndwt_plan_slab_fast: slab_fused3 for both directions at once, tap stride 1
                assert stride > 1 or row["fast"] == (both == FUSED3 or (both == FUSED3_T and mode == SLAB_Z)), (prm.id, both)
                for fam, params in picks:
                    rec = helpers._trace.KernelLaunch(fam, params)
                    assert any(helpers.matches(rec, sp) for sp in specs), (prm.id, (z0, z1), "syn" if inverse else "ana", rec, specs)
                    checked += 1
    assert checked >= 2 * 2 * 30


# every number of the two variant columns of csrc/ndwt_select.h (0: the default)
FWD_NUMBERS = (0, 1, 2, 3, 6, 7, 8, 9, 10, 11)
INV_NUMBERS = (0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12)


def test_every_pick_names_an_instance(shim):
    """fused3_select over everything level_route lets through -- both scalar types, real and interleaved complex, 3-D and 4-D, padded tap
    lengths 2 .. 20, uniform wavelets and mixed ones with even / odd padding (on y, so uniform_yz goes off, and on x, where it stays on),
    rows and pointers in whole groups of 4 scalars or not, volumes on both sides of the 32-tile threshold, the dilated levels (ew = dil = 2, 4),
    the folded t axis, every variant number of its direction: the pick is an entry of the instance lists (csrc/ndwt_fused_list.h), or the
    selector says that there is no kernel (the folded t axis on unaligned pointers; fwd 6 below 8 taps)"""
    picks, none = set(), 0
    for f64 in (False, True):
        for cplx in (False, True):
            comp = 2 if cplx else 1
            for L in range(2, 21, 2):
                mixes = [[L, L, L]] + ([[L, L - 2, L], [L - 2, L, L]] if L >= 4 else []) + ([[L, L - 4, L], [L - 4, L, L]] if L >= 6 else [])
                for lens in mixes:
                    for dims, stride in (([64, 40, 36], 1), ([70, 40, 36], 1), ([256, 256, 36], 1), ([64, 40, 36, 8], 1), ([72, 40, 36, 8], 1),
                                         ([64, 40, 36], 2), ([64, 40, 36], 4)):
                        for inverse in (False, True):
                            for number in (INV_NUMBERS if inverse else FWD_NUMBERS):
                                vf, vi = (0, number) if inverse else (number, 0)
                                plan = _plan(dims, lens + [4], f64, cplx, False, stride > 1, vf, vi)
                                kind, Lp = _route(shim, plan, stride, inverse)
                                if kind not in (FUSED3_DILATED, FUSED3, FUSED3_T, FUSED3_FOLD_T):
                                    continue
                                for vec4 in ((False, True) if (dims[0] * comp) % 4 == 0 else (False,)):
                                    tfold = kind == FUSED3_FOLD_T and vec4   # (unaligned pointers: the caller takes kRouteFused3T)
                                    if kind == FUSED3_DILATED:
                                        q = [f64, inverse, vec4, lens[1] == lens[2], 0, Lp] + lens + [stride, stride, dims[0], dims[1] // stride,
                                             stride * stride, vf, vi, NUM_CUS, 0]
                                    else:
                                        q = [f64, inverse, vec4, lens[1] == lens[2], tfold, Lp] + lens + [comp, 1, dims[0] * comp, dims[1],
                                             dims[3] if len(dims) == 4 else 1, vf, vi, NUM_CUS, 0]
                                    name, p, f = _fused3(shim, q)
                                    if name == "none":
                                        assert (vf == 6 and Lp < 8 and not f64 and not cplx) or (kind == FUSED3_FOLD_T and not vec4), q
                                        none += 1
                                        continue
                                    assert f["listed"], (name, p, q)
                                    assert (name == "Fwd3") == (not inverse)
                                    picks.add((name, tuple(sorted(p.items()))))
    # the sweep reaches the instances of every launch unit: by kernel, scalar type, x step and the flags that tell the units apart
    for fam, want in (("Fwd3", dict(T="float", PIN=True)), ("Fwd3", dict(T="float", TPRE=True)), ("Fwd3", dict(T="float", L=16, WLDS=2)),
                      ("Fwd3", dict(T="float", L=20, WLDS=4)), ("Fwd3", dict(T="float", L=20, WLDS=6)), ("Fwd3", dict(T="float", L=18, WLDS=2)),
                      ("Fwd3", dict(T="float", L=20, WLDS=0)), ("Fwd3", dict(T="float", EW=4)), ("Fwd3", dict(T="double", L=16, WLDS=2)),
                      ("Fwd3", dict(T="double", L=12, EW=2, WLDS=2)), ("Fwd3", dict(T="double", L=12, EW=2, WLDS=0)),
                      ("Inv3", dict(T="float")), ("Inv3", dict(T="double")), ("Inv3S", dict(T="float", L=16)), ("Inv3S", dict(T="float", EW=4)),
                      ("Inv3S", dict(T="float", EW=2)), ("Inv3S", dict(T="double", L=16)), ("Inv3S", dict(T="double", EW=2)),
                      ("Inv3Y", dict(XSC=True, EW=1, UNIYZ=True)), ("Inv3Y", dict(XSC=False, UNIYZ=True)), ("Inv3Y", dict(EW=2, XSC=True)),
                      ("Inv3Y", dict(EW=4, XSC=True)), ("Inv3Y", dict(EW=4, XSC=False)), ("Inv3Y", dict(L=12, ZLDS=6)), ("Inv3Y", dict(L=20, ZLDS=8)),
                      ("Inv3Y", dict(L=8, DEPTH=1, VEC4=False))):
        assert any(name == fam and all(dict(p).get(k) == v for k, v in want.items()) for name, p in picks), (fam, want)
    assert len(picks) >= 200 and none > 0, (len(picks), none)


def test_every_inv2p_pick_names_an_instance(shim):
    """fused2_select the same way against the Inv2P lists: both scalar types, tap lengths 2 .. 20, both sides of n2 >= 64 and of the one-round
    budget, every variant number"""
    seen = set()
    for f64 in (False, True):
        for L in range(2, 21, 2):
            for vec4 in (False, True):
                for n1, n2 in ((256, 63), (256, 64), (4096, 5250), (4096, 5251)):
                    for vi in INV_NUMBERS:
                        name, p, f = _fused2(shim, [f64, True, vec4, L, 1, 1, n1, n2, vi])
                        if name == "Inv2P":
                            assert f["listed"], (f64, L, vec4, n1, n2, vi, f)
                            seen.add((f64, L, p["PD"], p["PK"]))
    assert len(seen) == 12 + 4                                  # every entry of the two lists is some pick


# The route of a 2-D level by data kind, tap stride and tap length, written out (not computed from csrc/ndwt_fused_list.h): the longest
# fused tap length per (double, complex, stride); everything longer, and every kind and stride not named, takes the per-axis passes.
FUSED2_MAX_TAPS = {(False, False, 1): 20, (False, True, 1): 16, (True, False, 1): 16, (True, True, 1): 8,     # FUSED2
                   (False, False, 2): 8, (True, False, 2): 8, (False, False, 4): 8}                             # FUSED2_DILATED
N_FUSED2S = 136                                                 # Fwd2S / Inv2S kernels in the built library (nm -C libndwt_hip.so)


def test_every_fused2_pick_names_an_instance(shim):
    """level_route and fused2_select over the 2-D plans: both scalar types, real and interleaved complex, tap strides 1 / 2 / 4, tap lengths
    2 .. 20, both directions, rows in whole groups of 4 scalars or not, every variant number of the synthesis, images on both sides of
    n2 >= 64 and of the one-round budget.  The route is the literal table above; wherever it is fused, the pick is an entry of the
    instance lists; and the Fwd2S / Inv2S picks are the whole table, every kernel the library was built with (a pick with another
    WPE, or an instance no plan reaches, would break the count)"""
    reached = set()
    for f64 in (False, True):
        for cplx in (False, True):
            comp = 2 if cplx else 1
            for stride in (1, 2, 4):
                for L in range(2, 21, 2):
                    want = PER_AXIS if L > FUSED2_MAX_TAPS.get((f64, cplx, stride), 0) else FUSED2 if stride == 1 else FUSED2_DILATED
                    for n1, n2 in ((256, 63), (256, 64), (4096, 5250), (4096, 5251)):
                        dims = [n1, n2 if stride == 1 else n2 // 4 * 4]      # (a dilated level: both dims divisible by the stride)
                        for inverse in (False, True):
                            for vi in (INV_NUMBERS if inverse else (0,)):
                                plan = _plan(dims, [L, L], f64, cplx, False, stride > 1, 0, vi)
                                kind, Lp = _route(shim, plan, stride, inverse)
                                assert (kind, Lp) == (want, 0 if want == PER_AXIS else L), (f64, cplx, stride, L, dims, inverse, vi)
                                if kind == PER_AXIS:
                                    continue
                                ew = comp if stride == 1 else stride
                                for vec4 in (False, True):
                                    name, p, f = _fused2(shim, [f64, inverse, vec4, L, ew, stride, n1 * comp, dims[1], vi])
                                    assert f["listed"], (name, p, f)
                                    assert name == "Inv2P" or name == ("Inv2S" if inverse else "Fwd2S")
                                    if name != "Inv2P":
                                        reached.add((inverse, f64, vec4, L, ew, p["WPE"]))
    assert all(shim.sel_fused2s_listed(_ints(k)) for k in reached)
    assert len(reached) == N_FUSED2S, len(reached)
    # ... and no instance beside them: the lists over every name a pick could take
    listed = sum(shim.sel_fused2s_listed(_ints([inverse, f64, vec4, L, ew, wpe])) for inverse in (0, 1) for f64 in (0, 1) for vec4 in (0, 1)
                 for L in range(1, 25) for ew in (1, 2, 3, 4, 8) for wpe in (1, 2, 4, 8))
    assert listed == N_FUSED2S, listed


# ---- axes shorter than the dilated filter (tests/test_gpu_short_axes.py): the route of a level does not ask how long a sub-lattice is
def test_short_axis_levels_keep_their_routes(shim):
    """written out: [8, 8, 8] db4 runs the fused sub-lattice kernels at tap strides 2 and 4 (sub-lattices of 4 and 2 samples under 8
    taps) and the per-axis passes at 8; double has no stride-4 form; an axis the stride does not divide takes the per-axis passes"""
    for inverse in (False, True):
        f32 = _plan([8, 8, 8], [8, 8, 8], atrous=True)
        assert _route(shim, f32, 1, inverse) == (FUSED3, 8)
        assert _route(shim, f32, 2, inverse) == (FUSED3_DILATED, 8)
        assert _route(shim, f32, 4, inverse) == (FUSED3_DILATED, 8)
        assert _route(shim, f32, 8, inverse) == (PER_AXIS, 0)
        f64 = _plan([8, 8, 8], [8, 8, 8], f64=True, atrous=True)
        assert _route(shim, f64, 2, inverse) == (FUSED3_DILATED, 8)
        assert _route(shim, f64, 4, inverse) == (PER_AXIS, 0)
        assert _route(shim, _plan([8, 8, 8], [8, 8, 8], cplx=True, atrous=True), 2, inverse) == (PER_AXIS, 0)
        assert _route(shim, _plan([8, 8, 8], [8, 8, 8], generic=True, atrous=True), 2, inverse) == (PER_AXIS, 0)
        for dims, lens in (([16, 8, 8], [8, 8, 8]), ([12, 8, 8], [8, 8, 8]), ([8, 8, 4], [8, 8, 4]), ([8, 8, 8], [4, 8, 4]), ([8, 4, 4], [4, 4, 4]),
                           ([16, 8, 8], [6, 6, 6]), ([4, 4, 4], [2, 2, 2])):
            for stride in (2, 4):
                assert _route(shim, _plan(dims, lens, atrous=True), stride, inverse) == (FUSED3_DILATED, max(lens)), (dims, lens, stride)
        for stride in (2, 4):
            assert _route(shim, _plan([10, 9, 7], [6, 4, 4], atrous=True), stride, inverse) == (PER_AXIS, 0)
            assert _route(shim, _plan([16, 16, 8], [12, 12, 8], atrous=True), stride, inverse) == (PER_AXIS, 0)      # 12 taps: no sub-lattice form
            assert _route(shim, _plan([6, 4, 5, 4], [6, 4, 4, 2], atrous=True), stride, inverse) == (PER_AXIS, 0)
            assert _route(shim, _plan([9, 6], [4, 6], atrous=True), stride, inverse) == (PER_AXIS, 0)
            assert _route(shim, _plan([8, 8], [8, 8], atrous=True), stride, inverse) == (FUSED2_DILATED, 8)
            assert _route(shim, _plan([16, 4], [4, 4], atrous=True), stride, inverse) == (FUSED2_DILATED, 4)
        assert _route(shim, _plan([8, 8], [8, 8], f64=True, atrous=True), 2, inverse) == (FUSED2_DILATED, 8)
        assert _route(shim, _plan([8, 8], [8, 8], f64=True, atrous=True), 4, inverse) == (PER_AXIS, 0)


def test_short_axis_rows_route_and_pick_what_the_gpu_file_expects(shim):
    """every row of tests/test_gpu_short_axes.py on a plain plan, in every data kind it runs, level by level and both ways: the route
    that file's restatement of the selection rule gives is level_route's, and wherever the level is fused, fused3_select / fused2_select
    name a listed instance that one of the row's expected specs matches.  (Stacks, interleaved samples and batched plans: their own
    select tests; their dilated levels take the per-axis passes.)"""
    import test_gpu_short_axes as sa
    fused, checked = 0, 0
    for row in sa.ROWS:
        if row["plan"] != "plain":
            continue
        dims, lens, d = row["dims"], row["lens"], len(row["dims"])
        for kind in row["kinds"]:
            prec, cplx = sa.KINDS[kind]
            f64, comp = prec == "double", 2 if cplx else 1
            n1 = dims[0] * comp
            vec4 = not row["offset"] and n1 % 4 == 0 and (n1 * dims[1] if d > 1 else 4) % 4 == 0
            plan = _plan(dims, lens, f64, cplx, row["generic"], row["dil"] == "atrous", row["vf"], row["vi"])
            for inverse in (False, True):
                must, may = sa.expected(row, kind, inverse)
                specs = [helpers.spec(s) for s in must]
                for lev in range(1, row["level"] + 1):
                    stride = (1 << (lev - 1)) if row["dil"] == "atrous" else 1
                    kind_, Lp = _route(shim, plan, stride, inverse)
                    assert (kind_, Lp) == sa.level_kind(row, kind, stride, inverse), (row["id"], kind, stride, inverse, kind_, Lp)
                    checked += 1
                    if kind_ == PER_AXIS:
                        assert may or row["axis"], (row["id"], kind)
                        continue
                    if kind_ == FUSED3_DILATED:
                        name, p, f = _fused3(shim, [f64, inverse, vec4, lens[1] == lens[2], 0, Lp] + lens[:3] + [stride, stride, dims[0], dims[1] // stride,
                                                    stride * stride, row["vf"], row["vi"], NUM_CUS, 0])
                    elif kind_ in (FUSED3, FUSED3_T):
                        name, p, f = _fused3(shim, [f64, inverse, vec4, lens[1] == lens[2], 0, Lp] + lens[:3] + [comp, 1, n1, dims[1], dims[3] if d == 4 else 1,
                                                    row["vf"], row["vi"], NUM_CUS, 0])
                    else:
                        assert kind_ in (FUSED2, FUSED2_DILATED)
                        dil = stride if kind_ == FUSED2_DILATED else 1
                        left = row["level"] if row["dil"] == "reference" else 0
                        assert left == 0 or row["vf"] == row["vi"] == 11 or shim.sel_cascade2_levels(plan, inverse, left) == 0   # one launch per level
                        name, p, f = _fused2(shim, [f64, inverse, vec4, Lp, dil if dil > 1 else comp, dil, n1, dims[1], row["vi"]])
                    assert f["listed"], (row["id"], kind, name, p)
                    rec = helpers._trace.KernelLaunch(name, p)
                    assert not row["trace"] or any(helpers.matches(rec, sp) for sp in specs), (row["id"], kind, stride, "rec" if inverse else "dec", rec, must)
                    fused += 1
    assert checked >= 1000 and fused >= 400, (checked, fused)


def test_at_most_one_cascade_claims_a_plan_and_cascade_route_names_it(shim):
    """What the one walk of dec_impl / rec_impl rests on: over a grid of plans -- 1 to 4 axes, the four data kinds, plain, batched /
    stack, interleaved and both, both dilations, both paths, 2 .. 12 taps, every pair of the variants the cascades read, both
    directions, 1 .. 9 levels left, sizes on both sides of every floor the predicates test (rows of 8 L scalars, 3 (L - 1) image rows,
    24 MiB + 1 of float image, 256 MiB of interleaved samples) and rows that are not whole groups of 4 -- at most one of cascade1_levels,
    cascadem_levels and cascade2_levels answers a count, and cascade_route answers that family with its count and tap length, or
    kCascadeNone with zeros.  And kCascadeNone is final: where it is the answer for `left` levels it is the answer for fewer, so a walk
    that was told "none" need not ask again."""
    import numpy as np
    variants, nleft = [0, 9, 10, 11, 12], 9
    per_plan = len(variants) ** 2 * 2 * nleft
    out = (ctypes.c_int * (9 * per_plan))()
    shim.sel_cascade_routes.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    shim.sel_cascade_routes.restype = None
    seen, plans = np.zeros(4, dtype=np.int64), 0
    for ndim in (1, 2, 3, 4):
        for L in (2, 4, 6, 8, 10, 12):
            n0s = [8 * L, 8 * L - 4, 4 * L, 4 * L - 2, 63, 66, 512, 2048, 1 << 24, (1 << 24) - 4]
            n1s = [64] if ndim == 1 else [3 * (L - 1), 3 * (L - 1) - 1, 64, 3072, 3073] if ndim == 2 else [64, 3 * (L - 1)]
            for n0 in n0s:
                for n1 in n1s:
                    dims = ([n0, n1] + [8] * 2)[:ndim]
                    for f64 in (False, True):
                        for cplx in (False, True):
                            for howmany, inner in ((0, 1), (3, 1), (0, 4), (3, 4)):
                                for atrous in (False, True):
                                    for generic in (False, True):
                                        plan = _plan(dims, [L] * ndim, f64, cplx, generic, atrous)
                                        shim.sel_cascade_routes(plan, howmany, inner, _ints(variants), len(variants), nleft, out)
                                        a = np.frombuffer(out, dtype=np.int32).reshape(per_plan, 9)
                                        n, taps = a[:, 0:6:2], a[:, 1:6:2]
                                        what = (dims, L, f64, cplx, howmany, inner, atrous, generic)
                                        assert ((n > 0).sum(axis=1) <= 1).all(), what
                                        kind = (n > 0) @ np.array([1, 2, 3])               # CascadeKind: none, rows1, march, image2
                                        assert (a[:, 6] == kind).all() and (a[:, 7] == n.sum(axis=1)).all() and (a[:, 8] == taps.sum(axis=1)).all(), what
                                        assert ((a[:, 6] == 0) == (a[:, 7] == 0)).all() and (a[:, 7] <= np.tile(np.arange(1, nleft + 1), per_plan // nleft)).all(), what
                                        by_left = a[:, 6].reshape(-1, nleft)                # "none" is final: none at `left` levels, none at fewer
                                        assert ((by_left[:, 1:] != 0) | (by_left[:, :-1] == 0)).all(), what
                                        seen += np.bincount(a[:, 6], minlength=4)
                                        plans += 1
    assert plans >= 20000 and (seen > 0).all(), (plans, seen)                               # every family, and none, was among the answers


# ---- one pass along one axis: axis_select (csrc/ndwt_select.h), the pick axis_pass launches
MARCH, AXISX, PLAIN = helpers.AXIS_MARCH, helpers.AXIS_X, helpers.AXIS_PLAIN
Q = helpers.axis_query


def _axis(shim, *a, **kw):
    return helpers.axis_picks(shim, [Q(*a, **kw)])[0]


def test_axis_pick_on_both_sides_of_every_threshold(shim):
    """written out, one-level passes, both directions: the 1-D signal on both sides of n * comp = 8 L, of rows in whole groups of 4 on
    aligned pointers and of 12 taps; the per-axis path on request; interleaved samples in whole groups of 4 or not, aligned or not; a
    dilated pass on both sides of n / stride >= L and of s * inner in groups of 4; a slab pass; and the two grid limits"""
    for syn in (False, True):
        k = _axis(shim, 32, 4, syn=syn)                         # float db2: 32 = 8 * 4
        assert (k["kernel"], k["ew"], k["vec4"], k["row"], k["nseg"], k["grid"]) == (AXISX, 1, 1, 32, 1, 1), k
        assert _axis(shim, 31, 4, syn=syn)["kernel"] == PLAIN
        for k in (_axis(shim, 34, 4, syn=syn), _axis(shim, 32, 4, syn=syn, aligned=False)):
            assert (k["kernel"], k["vec4"], k["grid"]) == (AXISX, 0, 1), k
        k = _axis(shim, 24, 6, syn=syn, comp=2)                 # complex64 db3: 48 scalars = 8 * 6
        assert (k["kernel"], k["ew"], k["vec4"], k["row"]) == (AXISX, 2, 1, 48), k
        assert _axis(shim, 23, 6, syn=syn, comp=2)["kernel"] == PLAIN
        k = _axis(shim, 96, 12, syn=syn, f64=True)              # double db6
        assert (k["kernel"], k["row"], k["nseg"]) == (AXISX, 96, 1), k
        assert _axis(shim, 4096, 14, syn=syn, f64=True)["kernel"] == PLAIN            # db7: no AxisX beyond 12 taps
        k = _axis(shim, 4096, 4, syn=syn, path_auto=False)
        assert (k["kernel"], k["grid"]) == (PLAIN, 16), k
        k = _axis(shim, 40, 4, syn=syn, inner=4)                # interleaved samples of 4 scalars
        assert (k["kernel"], k["inner"], k["n"], k["n_in"], k["ngroups"], k["chunk"], k["nchunks"], k["grid"]) == (MARCH, 4, 40, 40, 1, 12, 4, 4), k
        assert _axis(shim, 40, 4, syn=syn, inner=3)["kernel"] == PLAIN
        assert _axis(shim, 40, 4, syn=syn, inner=4, aligned=False)["kernel"] == PLAIN
        assert _axis(shim, 32, 4, syn=syn, stride=2)["kernel"] == PLAIN               # 2 interleaved sub-lattices: no group of 4
        k = _axis(shim, 32, 4, syn=syn, stride=4)
        assert (k["kernel"], k["inner"], k["n"], k["n_in"], k["chunk"], k["nchunks"], k["grid"]) == (MARCH, 4, 8, 8, 8, 1, 1), k
        assert _axis(shim, 12, 4, syn=syn, stride=4)["kernel"] == PLAIN               # sub-lattices of 3 < 4 taps
        assert _axis(shim, 40, 4, syn=syn, inner=4, stride=2, wrap=False)["kernel"] == PLAIN
        k = _axis(shim, 40, 4, syn=syn, inner=4, wrap=False)
        assert (k["kernel"], k["n"], k["n_in"]) == (MARCH, 40, 43), k
        k = _axis(shim, 40, 4, syn=syn, inner=4, outer=(1 << 39) - 256)             # 256 rows to the workgroup, one chunk: 2^31 - 1 workgroups
        assert (k["kernel"], k["nchunks"], k["grid"]) == (MARCH, 1, (1 << 31) - 1), k
        k = _axis(shim, 40, 4, syn=syn, inner=4, outer=(1 << 39) - 255)             # ... and one more: the march is passed over

        assert (k["kernel"], k["grid"]) == (PLAIN, 256 * 64), k
        k = _axis(shim, (1 << 30) - 4, 4, syn=syn)
        assert (k["kernel"], k["row"]) == (AXISX, (1 << 30) - 4), k
        assert _axis(shim, 1 << 30, 4, syn=syn)["kernel"] == PLAIN


def _parent_axis_pass(f64, syn, path_auto, wrap, L, stride, comp, inner, n, outer, contiguous, aligned):
    """What axis_pass ran before axis_select existed, written down from its if-chain and from the -1 / -2 answers of the two launchers
    it tried in turn (launch_march: a switch over 2 .. 20 taps, a grid of 1 .. 2^31 - 1; launch_axisx: ew 1 or 2, a switch over 2 .. 12
    taps, segments of the kernel's WX, the same grid limit and rows below 2^30).  Returns the launch: kernel, grid and its arguments."""
    del f64
    top = (1 << 31) - 1
    m_inner, m_n, m_n_in = inner, n, (n if wrap else n + (L - 1) * stride)
    march_ok = bool(path_auto)
    if stride > 1:
        if wrap and n % stride == 0 and n // stride >= L:
            m_inner, m_n, m_n_in = inner * stride, n // stride, n // stride
        else:
            march_ok = False
    if march_ok and m_inner % 4 == 0 and m_inner >= 4 and aligned:
        ngroups = m_inner // 4
        iblocks = (ngroups * outer + 255) // 256
        want = max((4096 + iblocks - 1) // iblocks, 1)
        chunk = min(max((m_n + want - 1) // want, 4 * (L - 1), 8), m_n)
        nchunks = (m_n + chunk - 1) // chunk
        if L in (2, 4, 6, 8, 10, 12, 14, 16, 18, 20) and 0 < iblocks * nchunks <= top:
            return dict(kernel=MARCH, grid=iblocks * nchunks, inner=m_inner, n=m_n, n_in=m_n_in, ngroups=ngroups, chunk=chunk, nchunks=nchunks)
    if path_auto and contiguous and stride == 1 and wrap and L <= 12 and comp in (1, 2) and n * comp >= 8 * L:
        row = n * comp
        vec4 = row % 4 == 0 and bool(aligned)
        if L in (2, 4, 6, 8, 10, 12):
            lh, rh = (L // 2, L // 2 - 1) if syn else (L // 2 - 1, L // 2)
            wx = 4 * (64 - (lh * comp + 3) // 4 - (rh * comp + 3) // 4)            # AxisX::WX
            nseg = (row + wx - 1) // wx
            grid = (outer * nseg + 3) // 4
            if 0 < grid <= top and row < (1 << 30):
                return dict(kernel=AXISX, grid=grid, ew=comp, vec4=int(vec4), row=row, nseg=nseg)
    return dict(kernel=PLAIN, grid=min((outer * n * inner + 255) // 256, 256 * 64))


def test_axis_pick_is_the_parents_choice_over_a_sweep(shim):
    """axis_select over both scalar types, both directions, both paths, periodic or not, 2 .. 20 taps and the odd lengths between, real
    and interleaved complex, the contiguous axis or not, aligned or not, tap strides 1 .. 8, inner blocks of 1 .. 8 elements, axes on both
    sides of 8 L / comp, of L * stride and of the multiples of the stride, and three row counts: the pick is what the parent's axis_pass
    launched, field by field; it is in the instance lists; its chunks cover the axis exactly; its segments are wave_row_width's; and its
    grid is one the launch can express."""
    queries = []
    for L in list(range(2, 21, 2)) + [3, 13, 21, 22]:
        for comp in (1, 2):
            for stride in (1, 2, 4, 8):
                ns = sorted({8 * L // comp - 1, 8 * L // comp, L * stride - stride, L * stride, L * stride + 1, 8 * L * stride + 2 * stride, 4096})
                for n in ns:
                    for inner in (1, 2, 3, 4, 8):
                        for outer in (1, 3, 1 << 33):
                            for flags in range(64):
                                f64, syn, path_auto, wrap, contiguous, aligned = [(flags >> b) & 1 for b in range(6)]
                                queries.append([f64, syn, path_auto, wrap, L, stride, comp, comp * inner, n, outer, contiguous, aligned])
    assert len(queries) >= 100000
    seen = [0, 0, 0]
    for q, k in zip(queries, helpers.axis_picks(shim, queries)):
        want = _parent_axis_pass(*q)
        assert all(k[f] == v for f, v in want.items()), (dict(zip(helpers.AXIS_QUERY, q)), k, want)
        assert k["listed"], (q, k)
        assert 0 < k["grid"] <= (1 << 31) - 1, (q, k)
        if k["kernel"] == MARCH:
            assert (k["nchunks"] - 1) * k["chunk"] < k["n"] <= k["nchunks"] * k["chunk"] and k["ngroups"] * 4 == k["inner"], (q, k)
        if k["kernel"] == AXISX:
            assert k["nseg"] == -(-k["row"] // k["wx"]), (q, k)
        seen[k["kernel"]] += 1
    assert all(seen), seen                                      # all three kernels were among the answers


def test_axis_instance_lists_have_40_and_96_entries(shim):
    march = sum(shim.sel_axis_march_listed(f64, syn, L) for f64 in (0, 1) for syn in (0, 1) for L in range(1, 25))
    axisx = sum(shim.sel_axisx_listed(f64, syn, vec4, L, ew) for f64 in (0, 1) for syn in (0, 1) for vec4 in (0, 1) for L in range(1, 25)
                for ew in range(1, 5))
    assert (march, axisx) == (40, 96)
