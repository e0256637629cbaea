"""The oracle, held to the reference's own C code.

mex/nddwt.c of the reference is plain C99 over seven FFTW symbols.  `make -C oracle ref` (called by build()) compiles it unchanged against
oracle/ref/ -- a plain long-double DFT behind those symbols -- into oracle/_ref/libnddwt_ref.so, and oracle/ndwt_ref.py drives it the way
the MATLAB class drives nd_dwt_mex (Functions/nd_dwt_3D.m:157-161,217-225; level 1 / level > 1 as nd_dwt_mex.c:90-98,141-148).  Here:

  * the DFT stand-in alone, against numpy.fft.fftn (<= 1e-14 max|X|, numpy's own error at these lengths): if the reference and the
    oracle ever disagree because of the stand-in, this test shows it first;
  * the compiled reference against all four restatements of the transform: the nddwt.c control flow in numpy (mex_dec / mex_dec_1level /
    mex_rec behind NdDwtMex, <= 1e-13 max|c|, the bound of tests/test_reference_pins.py between restatements), the 'mat' path NdDwtMat,
    the signal-domain numpy form and oracle/ndwt_spatial.c in double (<= 1e-12 max|c| each) -- written-out cases, the shapes of the
    reference's own scripts at a tenth, and a seeded sweep.  The reference has no a-trous mode, so none of this runs dilated;
  * tests/golden/d*.npz (written by our oracle) reproduced by the reference, so those fixtures are pinned to it as well;
  * the reference's acceptance invariants on its own output (Test/nddwt3D_test.m:25-27);
  * tests/golden/refc/*.npz -- written BY the reference, tests/golden/make_golden_refc.py -- reproduced by every restatement.  This
    test needs no library and never skips; where the library is present the fixtures are regenerated and compared as well.

What this pins: the C control flow of nddwt.c given the kernels (band slots, level order nddwt.c:209-234, the conjugate of :163, where
1/2^d goes :176-182, the last-level branch :277).  Still restated: the MATLAB side (get_filters, the fftn around the call, the 'mat'
path), nd_dwt_mex.c and the prebuilt mex binaries.

Tests that need the library FAIL where a reference checkout exists and the library does not (the build is broken), and skip where
both are missing.  error = max|got - want| / max|c|, c the coefficients of the call (dec: its output, rec: its input).
"""
import glob
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import ndwt_oracle as orc
import ndwt_ref as ref
import ndwt_spatial as orc_c

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BOUND = {"mex": 1e-13, "mat": 1e-12, "spatial": 1e-12, "spatial_c": 1e-12}
WORST = {k: 0.0 for k in BOUND}


def need_lib():
    """first line of every test that calls the compiled reference"""
    if not ref.available():
        if os.path.isdir(ref.reference_dir()):
            pytest.fail(f"the reference is at {ref.reference_dir()} but {ref.LIB_PATH} is missing: `make -C oracle ref` (build()) is broken")
        pytest.skip("no reference checkout and no oracle/_ref/libnddwt_ref.so")
    ref.load()


@pytest.fixture(scope="module", autouse=True)
def print_worst():
    yield
    if ref.available():
        print("\n[reference-c] worst error against the compiled reference, relative to max|c|: "
              + ", ".join(f"{k} {WORST[k]:.3g} (bound {BOUND[k]:.0e})" for k in BOUND))


# ---------------------------------------------------------------------------------------------------------------------------------
# the DFT stand-in alone
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rank", [1, 2, 3, 4])
@pytest.mark.parametrize("n", [1, 2, 3, 7, 16, 37, 54, 131])
def test_dft_stand_in_against_numpy(n, rank):
    """length n on every axis position of a rank-dimensional plan (the other axes 3, 2, 5), howmany 1 and 8, the forward call and the
    pointer-swapped call of nddwt.c:128,164 (the unnormalised inverse)"""
    need_lib()
    rng = np.random.default_rng(1000 * n + rank)
    others = [3, 2, 5]
    worst = 0.0
    for pos in range(rank):
        shape = others[:rank - 1]
        shape.insert(pos, n)
        for howmany in (1, 8):
            a = rng.standard_normal(shape + [howmany]) + 1j * rng.standard_normal(shape + [howmany])
            axes = tuple(range(rank))
            for inverse in (False, True):
                want = np.fft.ifftn(a, axes=axes) * np.prod(shape) if inverse else np.fft.fftn(a, axes=axes)
                got = ref.shim_dft(a, rank, howmany, inverse)
                err = np.abs(got - want).max() / np.abs(want).max()
                worst = max(worst, err)
                assert err <= 1e-14, (shape, howmany, inverse, err)
    print(f"[reference-c] dft n={n} rank={rank}: worst {worst:.3g} of max|X| (bound 1e-14)")


# ---------------------------------------------------------------------------------------------------------------------------------
# the compiled reference against the four restatements
# ---------------------------------------------------------------------------------------------------------------------------------
def _data(rng, shape, cplx):
    return rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if cplx else 0)


def _restatements_dec(x, wn, level, l2):
    sizes = list(x.shape)
    return {"mex": orc.NdDwtMex(wn, sizes, l2).dec(x, level), "mat": orc.NdDwtMat(wn, sizes, l2).dec(x, level),
            "spatial": orc.spatial_dec(x, wn, level, l2, "reference"), "spatial_c": orc_c.spatial_dec(x, wn, level, l2, "reference")}


def _restatements_rec(c, wn, l2):
    sizes = list(c.shape[:-1])
    return {"mex": orc.NdDwtMex(wn, sizes, l2).rec(c), "mat": orc.NdDwtMat(wn, sizes, l2).rec(c),
            "spatial": orc.spatial_rec(c, wn, l2, "reference"), "spatial_c": orc_c.spatial_rec(c, wn, l2, "reference")}


def _hold(got, ref_out, scale, what):
    for k, v in got.items():
        assert v.shape == ref_out.shape and v.dtype == ref_out.dtype, (what, k, v.shape, v.dtype, ref_out.shape, ref_out.dtype)
        err = float(np.abs(v - ref_out).max() / scale)
        WORST[k] = max(WORST[k], err)
        assert err <= BOUND[k], (what, k, err)


def check_config(sizes, wn, level, l2, cplx, seed):
    """dec(x) and rec of arbitrary coefficients by the compiled reference, against every restatement"""
    rng = np.random.default_rng(seed)
    what = (sizes, wn, level, l2, cplx)
    x = _data(rng, sizes, cplx)
    y = ref.dec(x, wn, level, l2)
    assert y.shape == tuple(sizes) + (orc.num_bands(len(sizes), level),) and np.iscomplexobj(y) == bool(cplx)
    _hold(_restatements_dec(x, wn, level, l2), y, np.abs(y).max(), ("dec",) + what)
    c = _data(rng, y.shape, cplx)
    r = ref.rec(c, wn, l2)
    _hold(_restatements_rec(c, wn, l2), r, np.abs(c).max(), ("rec",) + what)
    return x, y


def _all_settings(sizes, wn, seed, levels=(1, 2, 4)):
    for level in levels:                 # the single-level calls, nd_dwt_dec / nd_dwt_rec, and the latter's last-level branch (nddwt.c:277)
        for l2 in (0, 1):
            for cplx in (False, True):
                check_config(sizes, wn, level, l2, cplx, seed + 100 * level + 10 * l2 + cplx)


@pytest.mark.parametrize("K", range(1, 11))
def test_reference_c_1d_every_filter_on_the_shortest_axes(K):
    """db1 .. db10 at n = 2K, the shortest axis get_filters accepts (nd_dwt_1D.m: the filter must fit), and at n = 2K + 3"""
    need_lib()
    for n in (2 * K, 2 * K + 3):
        _all_settings([n], f"db{K}", 7000 + 50 * K + n)


WRITTEN = [
    ([12, 10], ["db1", "db3"]), ([11, 13], "db4"),
    ([8, 7, 6], ["db1", "db3", "db2"]), ([10, 9, 8], "db4"), ([20, 17, 12], ["db10", "db1", "db5"]),
    ([5, 6, 4, 5], ["db1", "db3", "db1", "db2"]),
]


@pytest.mark.parametrize("sizes,wn", WRITTEN, ids=["x".join(map(str, s)) for s, _ in WRITTEN])
def test_reference_c_written_out_cases(sizes, wn):
    need_lib()
    _all_settings(sizes, wn, 8000 + sum(sizes))


# the reference's own scripts with every axis at a tenth: Test/nddwt{1,2,3,4}D_test.m:5-11 (wavelets, level, pres_l2_norm and complex
# randn input as there) and mex/mex_test.m:4,11-13,48-49,84-85,120-121 (level 1, db1 in 1-D .. 3-D, db3 in 4-D; both l2 settings here)
SCRIPTS = [
    ("nddwt1D_test", [5433], "db1", 4, (0,)),
    ("nddwt2D_test", [27, 26], ["db1", "db3"], 1, (1,)),
    ("nddwt3D_test", [17, 7, 4], ["db1", "db3", "db1"], 1, (1,)),
    ("nddwt4D_test", [7, 7, 2, 2], ["db1", "db3", "db1", "db1"], 1, (1,)),
    ("mex_test-1D", [1000], "db1", 1, (0, 1)),
    ("mex_test-2D", [13, 14], "db1", 1, (0, 1)),
    ("mex_test-3D", [14, 13, 3], "db1", 1, (0, 1)),
    ("mex_test-4D", [13, 7, 6, 6], "db3", 1, (0, 1)),
]


@pytest.mark.parametrize("name,sizes,wn,level,l2s", SCRIPTS, ids=[s[0] for s in SCRIPTS])
def test_reference_c_on_the_shapes_of_its_own_scripts(name, sizes, wn, level, l2s):
    need_lib()
    for l2 in l2s:
        check_config(sizes, wn, level, l2, True, 9000 + sum(sizes) + l2)


def sweep_cases(n, seed):
    """`n` random configurations from a fixed seed, in the manner of helpers.fuzz_cases without its a-trous branch (the reference has no
    dilation) and on axes short enough for an O(n^2) DFT: 1-D to 4-D, db1 .. db10 mixed per axis, axes from the shortest legal one,
    levels 1 .. 4, both pres_l2_norm settings, real and complex data"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        d = int(rng.choice([1, 2, 3, 3, 4]))
        budget = {1: 600, 2: 40, 3: 16, 4: 9}[d]
        orders = [int(rng.integers(1, min(10, budget // 2) + 1)) for _ in range(d)]
        sizes = [int(rng.integers(2 * o, max(2 * o + 2, budget))) for o in orders]
        out.append(dict(sizes=sizes, wn=[f"db{o}" for o in orders], level=int(rng.integers(1, 5)), l2=int(rng.integers(0, 2)),
                        cplx=bool(rng.random() < 0.5), seed=int(seed) * 100003 + k))
    return out


SWEEP = sweep_cases(120, seed=20261020)


@pytest.mark.parametrize("chunk", range(6))
def test_reference_c_seeded_sweep(chunk):
    """120 configurations, 20 to a test"""
    need_lib()
    for c in SWEEP[20 * chunk:20 * chunk + 20]:
        check_config(c["sizes"], c["wn"], c["level"], c["l2"], c["cplx"], c["seed"])


def test_sweep_reaches_every_dimension_level_and_filter():
    assert len(SWEEP) >= 100
    assert {len(c["sizes"]) for c in SWEEP} == {1, 2, 3, 4} and {c["level"] for c in SWEEP} == {1, 2, 3, 4}
    assert {w for c in SWEEP for w in c["wn"]} == {f"db{k}" for k in range(1, 11)}
    assert {(c["l2"], c["cplx"]) for c in SWEEP} == {(0, False), (0, True), (1, False), (1, True)}


# ---------------------------------------------------------------------------------------------------------------------------------
# the fixtures our oracle wrote: from here on pinned to the reference too
# ---------------------------------------------------------------------------------------------------------------------------------
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "d*.npz")))


def _wname(g):
    wn = [str(w) for w in g["wname"]]
    return wn[0] if len(wn) == 1 else wn


def test_the_five_oracle_fixtures_are_all_here():
    assert len(GOLDEN) == 5


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_reference_c_reproduces_the_oracle_fixtures(path):
    """every y_*_l2* and rec_*_l2* array of tests/golden/d*.npz (the *_atrous keys aside: the reference has no such mode)"""
    need_lib()
    g = np.load(path)
    wn, level = _wname(g), int(g["level"])
    keys = [k for k in g.files if (k.startswith("y_") or k.startswith("rec_")) and not k.endswith("_atrous")]
    assert len(keys) == 6, keys
    for k in keys:
        kind, tag, l2 = k.split("_")
        l2 = int(l2[2:])
        got = ref.dec(g[f"x_{tag}"], wn, level, l2) if kind == "y" else ref.rec(g[f"c_{tag}"], wn, l2)
        scale = np.abs(g[k]).max() if kind == "y" else np.abs(g[f"c_{tag}"]).max()
        assert got.shape == g[k].shape and got.dtype == g[k].dtype
        err = float(np.abs(got - g[k]).max() / scale)
        assert err <= 1e-12, (os.path.basename(path), k, err)


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference's own acceptance invariants, on its own output (Test/nddwt3D_test.m:25-27): round trip, and energy in l2 mode
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,wn,level", [([41], "db5", 4), ([12, 10], ["db1", "db3"], 2), ([10, 9, 8], "db4", 3),
                                            ([5, 6, 4, 5], ["db1", "db3", "db1", "db2"], 2), ([17, 7, 4], ["db1", "db3", "db1"], 1)])
def test_reference_c_invariants_on_its_own_output(sizes, wn, level):
    """rec(dec(x)) = x in both normalisations; ||dec(x)|| = ||x|| with pres_l2_norm.  1e-12: an orthonormal filter bank per level and
    axis, double arithmetic -- a few hundred roundings of 1.1e-16 at most"""
    need_lib()
    rng = np.random.default_rng(sum(sizes) + level)
    for cplx in (False, True):
        x = _data(rng, sizes, cplx)
        for l2 in (0, 1):
            y = ref.dec(x, wn, level, l2)
            r = ref.rec(y, wn, l2)
            assert r.dtype == x.dtype and np.abs(r - x).max() <= 1e-12 * np.abs(x).max(), (sizes, l2, cplx)
            if l2:
                assert abs(np.linalg.norm(y) - np.linalg.norm(x)) <= 1e-12 * np.linalg.norm(x), (sizes, cplx)


# ---------------------------------------------------------------------------------------------------------------------------------
# fixtures written by the reference: tests/golden/refc/*.npz
# ---------------------------------------------------------------------------------------------------------------------------------
REFC = sorted(glob.glob(os.path.join(HERE, "golden", "refc", "*.npz")))


def _load_generator():
    spec = importlib.util.spec_from_file_location("make_golden_refc", os.path.join(HERE, "golden", "make_golden_refc.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_reference_fixtures_are_all_here():
    """5 cases, real and complex: never empty, so the tests below cannot pass by running on nothing"""
    names = [os.path.basename(p)[:-4] for p in REFC]
    want = [f"{n}_{t}" for n in ("d1_n37_db2_L3", "d1_n40_db10_L2", "d2_12x10_db1db3_L2", "d3_10x9x8_db4_L3", "d4_5x6x4x5_mixed_L2")
            for t in ("r", "c")]
    assert sorted(names) == sorted(want)
    for p in REFC:
        assert os.path.getsize(p) < (1 << 20), p
        g = np.load(p)
        tag = os.path.basename(p)[:-4][-1]
        assert sorted(g.files) == sorted(["sizes", "level", "wname", f"x_{tag}", f"c_{tag}"] + [f"{a}_{tag}_l2{l2}" for a in ("y", "rec") for l2 in (0, 1)])


@pytest.mark.parametrize("path", REFC, ids=[os.path.basename(p)[:-4] for p in REFC])
def test_every_restatement_reproduces_the_reference_fixtures(path):
    """no library needed: the stored reference output against mex_dec / mex_rec, NdDwtMat, the signal-domain form and ndwt_spatial.c"""
    g = np.load(path)
    tag = os.path.basename(path)[:-4][-1]
    wn, level = _wname(g), int(g["level"])
    x, c = g[f"x_{tag}"], g[f"c_{tag}"]
    assert np.iscomplexobj(x) == (tag == "c") and list(x.shape) == [int(s) for s in g["sizes"]]
    for l2 in (0, 1):
        y, r = g[f"y_{tag}_l2{l2}"], g[f"rec_{tag}_l2{l2}"]
        for k, v in _restatements_dec(x, wn, level, l2).items():
            assert v.shape == y.shape and v.dtype == y.dtype
            err = float(np.abs(v - y).max() / np.abs(y).max())
            assert err <= BOUND[k], (os.path.basename(path), "dec", l2, k, err)
        for k, v in _restatements_rec(c, wn, l2).items():
            assert v.shape == r.shape and v.dtype == r.dtype
            err = float(np.abs(v - r).max() / np.abs(c).max())
            assert err <= BOUND[k], (os.path.basename(path), "rec", l2, k, err)


def test_reference_c_regenerates_its_fixtures():
    """the generator, run again in memory: <= 1e-15 max|c| (not equal bits -- long double is not the same on every host)"""
    need_lib()
    gen = _load_generator()
    assert len(REFC) == 2 * len(gen.CASES)
    for path in REFC:
        base = os.path.basename(path)[:-4]
        g, new = np.load(path), gen.generate(base[:-2], base[-1])
        assert sorted(g.files) == sorted(new)
        tag = base[-1]
        for k in g.files:
            if k in ("sizes", "level", "wname") or k.startswith("x_") or k.startswith("c_"):
                assert np.array_equal(g[k], new[k]), (base, k)
            else:
                scale = np.abs(g[k]).max() if k.startswith("y_") else np.abs(g[f"c_{tag}"]).max()
                assert np.abs(g[k] - new[k]).max() <= 1e-15 * scale, (base, k, np.abs(g[k] - new[k]).max() / scale)


# ---------------------------------------------------------------------------------------------------------------------------------
def test_nothing_of_the_compiled_reference_is_tracked():
    """oracle/_ref/ holds code compiled from the reference: never committed"""
    try:
        inside = subprocess.run(["git", "-C", ROOT, "rev-parse", "--is-inside-work-tree"], capture_output=True, text=True)
    except FileNotFoundError:
        pytest.skip("no git")
    if inside.returncode != 0 or inside.stdout.strip() != "true":
        pytest.skip("not a git work tree")
    tracked = subprocess.run(["git", "-C", ROOT, "ls-files", "oracle/_ref"], capture_output=True, text=True, check=True).stdout.split()
    assert tracked == []
