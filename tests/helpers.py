"""Shared helpers of the test-suite (CPU side)."""
import numpy as np

import ndwt_oracle as orc


def kernel_taps(wname, pres_l2_norm, Lp=None):
    """Kernel-form taps of one axis (what csrc/ndwt_filters.h:make_axis_filter builds), zero-padded to Lp."""
    lo_d, hi_d = orc.wave_filters(wname)
    L = len(lo_d)
    c = 1 / np.sqrt(2.0) if pres_l2_norm else 1.0
    cs = 1 / np.sqrt(2.0) if pres_l2_norm else 0.5
    t = {"ana_lo": c * lo_d[::-1], "ana_hi": c * hi_d[::-1], "syn_lo": cs * lo_d, "syn_hi": cs * hi_d}
    if Lp is not None:
        pad = (Lp - L) // 2
        t = {k: np.concatenate([np.zeros(pad), v, np.zeros(pad)]) for k, v in t.items()}
    return t


def to_kernel_order(x_mat):
    """MATLAB-shaped array [n1,...,nd(,bands)] -> C-contiguous [(bands,) nd, ..., n1] (column-major memory)."""
    return np.ascontiguousarray(np.transpose(x_mat))


def from_kernel_order(a):
    return np.transpose(a)


def fuzz_cases(n, seed, max_order=10, p_atrous=0.2):
    """`n` random transform configurations from a fixed seed (the generator of tools/fuzz_gpu.py): dimensions (primes,
    sizes below one tile, ragged tiles), mixed db1..db10 wavelets, levels, precisions, real / complex, both dilations.
    Returns dicts; the per-case data seed is part of the dict so that a single case can be replayed."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        d = int(rng.choice([1, 2, 3, 3, 3, 4]))
        budget = {1: 5000, 2: 90, 3: 40, 4: 14}[d]
        orders = [int(rng.integers(1, min(max_order, 10 if d < 4 else 4) + 1)) for _ in range(d)]
        sizes = [int(rng.integers(2 * o, max(2 * o + 2, budget))) for o in orders]
        if rng.random() < 0.3:
            sizes[0] = int(rng.choice([64, 68, 72, 128, 132])) if d <= 3 else sizes[0]      # whole tiles / ragged tiles
        level = int(rng.integers(1, 4))
        dilation = "atrous" if rng.random() < p_atrous else "reference"
        if dilation == "atrous":                                 # dilated filters (plans are built for 3 levels) must fit the axis
            orders = [min(o, 3 if d < 4 else 2) for o in orders]
            sizes = [max(s, 2 * o * 4) for s, o in zip(sizes, orders)]
            if rng.random() < 0.7:                               # axes that divide by 4: dilated levels run fused on sub-lattices
                sizes = [4 * ((s + 3) // 4) for s in sizes]
        out.append({"d": d, "sizes": sizes, "wn": [f"db{o}" for o in orders], "level": level, "dilation": dilation,
                    "l2": int(rng.integers(0, 2)), "precision": "single" if rng.random() < 0.5 else "double",
                    "cplx": bool(rng.random() < 0.4), "data_seed": int(seed) * 100003 + k})
    return out


def short_axis_cases(n, seed):
    """`n` random configurations on the shortest legal axes (a generator of its own beside fuzz_cases, same dicts): every axis has
    L .. L + 3 samples for its filter of L taps, a-trous dilation with probability 1/2 at 1 .. 4 levels -- so a dilated filter is longer
    than its axis, wraps round it more than once, lands two taps on one sample or (tap stride a multiple of the axis) all of them --,
    the four data kinds, both pres_l2_norm settings"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        d = int(rng.choice([1, 2, 3, 3, 4]))
        orders = [int(rng.integers(1, (10 if d < 4 else 4) + 1)) for _ in range(d)]
        sizes = [2 * o + int(rng.integers(0, 4)) for o in orders]
        out.append({"d": d, "sizes": sizes, "wn": [f"db{o}" for o in orders], "level": int(rng.integers(1, 5)),
                    "dilation": "atrous" if rng.random() < 0.5 else "reference", "l2": int(rng.integers(0, 2)),
                    "precision": "single" if rng.random() < 0.5 else "double", "cplx": bool(rng.random() < 0.5),
                    "data_seed": int(seed) * 100003 + k})
    return out


def zero_bands(sizes, level, dilation):
    """bands of a `level`-level transform that are identically zero in exact arithmetic: a-trous details of a level whose tap stride is
    a multiple of an axis on which they are high-pass (every tap lands on one sample, and the high-pass taps sum to zero).  Band order
    of the reference: 0 = approximation, then the details of the coarsest level first; bit a of a detail's number = high-pass on axis a"""
    d = len(sizes)
    nd = (1 << d) - 1
    zero = np.zeros(1 + nd * level, dtype=bool)
    if dilation == "atrous":
        for lev in range(1, level + 1):
            stride = 1 << (lev - 1)
            for bits in range(1, nd + 1):
                zero[1 + nd * (level - lev) + bits - 1] = any((bits >> a) & 1 and stride % sizes[a] == 0 for a in range(d))
    return zero


def fuzz_id(c):
    return (f"{c['d']}d-{'x'.join(map(str, c['sizes']))}-{'.'.join(w[2:] for w in c['wn'])}-L{c['level']}-l2{c['l2']}-"
            f"{c['precision'][0]}{'c' if c['cplx'] else 'r'}-{c['dilation'][0]}")


# ---- launch trace (non-decimated_wavelets_amd/trace.py): expected kernels of a call, and the coverage list of the dispatch tests
from importlib import import_module as _imp                                        # noqa: E402

_trace = _imp("non-decimated_wavelets_amd.trace")
parse_record = _trace.parse_record


def spec(s):
    """"Fwd3 L=8 TY=32 PIN=false" -> ("Fwd3", {"L": 8, "TY": 32, "PIN": False}): a family and the parameters that pick the branch"""
    fam, *kv = s.split()
    return fam, {k: _trace._value(v) for k, v in (p.split("=") for p in kv)}


def matches(rec, sp):
    fam, params = sp
    return rec.family == fam and all(rec.params.get(k) == v for k, v in params.items())


def check_trace(recs, specs, what=""):
    """every spec was launched at least once, and every launch is one of the specs (a dispatch change fails here, loudly)"""
    sps = [spec(s) for s in specs]
    shown = "\n  ".join(map(repr, recs)) or "(nothing launched)"
    for s, sp in zip(specs, sps):
        assert any(matches(r, sp) for r in recs), f"{what}: no launch of [{s}]; launched:\n  {shown}"
    for r in recs:
        assert any(matches(r, sp) for sp in sps), f"{what}: unexpected launch {r!r}; expected {specs}; launched:\n  {shown}"


# ---- kernel selection on the host: csrc/ndwt_select.h behind C entry points (tests/select/select_shim.cpp), compiled with g++
def build_select_shim(outdir):
    import ctypes
    import os
    import subprocess
    out = os.path.join(outdir, "libselect_shim.so")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "select", "select_shim.cpp")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", src, "-o", out], check=True)
    lib = ctypes.CDLL(out)
    lib.sel_fused3.restype = ctypes.c_char_p
    return lib


AXIS_MARCH, AXIS_X, AXIS_PLAIN = range(3)                      # AxisKernel of csrc/ndwt_select.h
AXIS_QUERY = ("f64", "syn", "path_auto", "wrap", "L", "stride", "comp", "inner", "n", "outer", "contiguous", "aligned")
AXIS_PICK = ("kernel", "grid", "inner", "n", "n_in", "ngroups", "chunk", "nchunks", "ew", "vec4", "row", "nseg", "wx", "listed")


def axis_query(n, L=4, f64=False, syn=False, path_auto=True, wrap=True, stride=1, comp=1, inner=None, outer=1, contiguous=None, aligned=True):
    """an AxisQuery as the 12 integers of sel_axis: one pass of `L` taps along an axis of `n` in the view [outer][n][inner] (inner in
    scalars; default: the contiguous axis of a plan without interleaved samples, inner = comp)"""
    inner = comp if inner is None else inner
    contiguous = inner == comp if contiguous is None else contiguous
    return [int(v) for v in (f64, syn, path_auto, wrap, L, stride, comp, inner, n, outer, contiguous, aligned)]


def axis_picks(shim, queries):
    """axis_select for every query: a list of dicts over AXIS_PICK (wx: wave_row_width of the query, listed: the instance lists hold the pick)"""
    import ctypes
    n = len(queries)
    flat = (ctypes.c_longlong * (12 * n))(*[v for q in queries for v in q])
    out = (ctypes.c_longlong * (14 * n))()
    shim.sel_axis_many(flat, ctypes.c_longlong(n), out)
    return [dict(zip(AXIS_PICK, out[14 * i:14 * i + 14])) for i in range(n)]


def axis_launch(q, k):
    """the launch record a pick stands for, as the trace spells it: (family, parameters, grid)"""
    T, syn = ("double" if q[0] else "float"), bool(q[1])
    if k["kernel"] == AXIS_MARCH:
        return "AxisMarch", {"T": T, "L": q[4], "SYN": syn}, k["grid"]
    if k["kernel"] == AXIS_X:
        return "AxisX", {"T": T, "L": q[4], "SYN": syn, "EW": k["ew"], "VEC4": bool(k["vec4"])}, k["grid"]
    return ("axis_synthesis_kernel" if syn else "axis_analysis_kernel"), {"T": T}, k["grid"]


# Every kernel family of csrc/ndwt_device.h and every plain __global__ kernel of csrc/, with the instances that tell the dispatcher's
# branches apart.  tests/test_gpu_dispatch.py::test_dispatch_coverage runs a sweep that must launch each entry (and agree with the
# oracle); tests/test_kernel_trace.py keeps the set of families here equal to the kernels in csrc/.
COVERAGE = [spec(s) for s in [
    "Fwd3 VEC4=true", "Fwd3 VEC4=false", "Fwd3 TY=16", "Fwd3 TY=32", "Fwd3 PIN=true", "Fwd3 TPRE=true", "Fwd3 LOWONLY=true",
    "Fwd3 WLDS=2", "Fwd3 WLDS=4", "Fwd3 EW=1", "Fwd3 EW=2", "Fwd3 EW=4", "Fwd3 T=double", "Fwd3 T=double EW=2",
    "Inv3 L=8",
    "Inv3S EW=1", "Inv3S EW=2", "Inv3S EW=4", "Inv3S T=double", "Inv3S L=16",
    "Inv3Y XSC=false", "Inv3Y XSC=true", "Inv3Y UNIYZ=true", "Inv3Y UNIYZ=false", "Inv3Y EW=1", "Inv3Y EW=2", "Inv3Y EW=4",
    "Inv3Y VEC4=true", "Inv3Y VEC4=false", "Inv3Y TX=48", "Inv3Y EW=2 XSC=true", "Inv3Y EW=4 XSC=true",
    "Den3",
    "Fwd2S VEC4=true", "Fwd2S VEC4=false", "Fwd2S EW=2", "Fwd2S EW=4", "Fwd2S T=double",
    "Fwd2C NLEV=2", "Fwd2C NLEV=3",
    "Inv2S VEC4=true", "Inv2S VEC4=false", "Inv2S EW=2", "Inv2S EW=4", "Inv2S T=double",
    "Inv2P PK=true", "Inv2P PK=false", "Inv2P T=double",
    "Inv2C NLEV=2", "Inv2C NLEV=3", "Inv2C PD=2",
    "AxisMarch SYN=false", "AxisMarch SYN=true",
    "AxisX VEC4=true", "AxisX VEC4=false", "AxisX EW=2",
    "axis_analysis_kernel", "axis_synthesis_kernel", "shrink_kernel", "segments_kernel", "segments_strided_kernel", "add_planes_kernel",
]]
