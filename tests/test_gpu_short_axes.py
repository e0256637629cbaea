"""Axes shorter than the filter's reach, on every route of the device.

Plan creation accepts an axis whenever the un-dilated filter fits it.  Under a-trous dilation level j steps its taps by 2^(j-1): its
filter of (L - 1) 2^(j-1) + 1 samples goes round a short axis more than once, and two taps (tap stride a multiple of the axis: all of
them) land on one sample.  At the reference's dilation the same happens wherever an axis is shorter than the PADDED taps of a fused
kernel (mixed wavelets) and, barely not, at n == L.  Four groups of rows:

  a. a-trous levels on the fused sub-lattice kernels (Fwd3 / Inv3Y / Inv3S / Fwd2S / Inv2S with EW = 2 / 4) whose sub-lattices have 4, 2
     or 1 samples under up to 8 padded taps; synthesis variants 4 / 5 / 10; coefficient and output pointers off by one element;
  b. a-trous levels on the per-axis passes: axes the stride does not divide, axes it divides into fewer than L samples (no AxisMarch),
     complex data, 4-D, tap strides >= the axis, the per-axis path on request;
  c. batched 1-D plans, stacks and interleaved samples, a-trous and short: items one by one, guard elements, ndwt_denoise_bands soft
     and hard against numpy shrinkage of the oracle's coefficients;
  d. the reference's dilation at n == L for db1 .. db10 in 1-D / 2-D / 3-D, axes of 2 and 4 under 20 padded taps, the AxisX threshold
     n * comp = 8 L, variant 11 / 11 on the 2-D and batched rows;
  and a fixed subset of helpers.short_axis_cases through the classes.

Every row: four data kinds, both pres_l2_norm settings, fp64 numpy oracle on standard_normal data of a fixed seed, the bounds of
tests/test_gpu_parity.py (TOL relative to max|want|: dec <= TOL, rec of random coefficients <= 4 TOL, rec(dec(x)) <= 20 TOL); bands that
are identically zero in exact arithmetic (helpers.zero_bands) are compared as max|got| <= TOL max|x|.  Every call runs inside
ndwt.kernel_trace(); the kernels expected are a restatement of csrc/ndwt_select.h (level_kind / expected below), which
tests/test_dispatch_select.py checks against the header itself without a device.
"""
import zlib

import numpy as np
import pytest
import torch

import helpers
import ndwt_amd as ndwt
import ndwt_oracle as orc

pytestmark = pytest.mark.gpu

TOL = {"double": 1e-12, "single": 2e-6}                       # tests/test_gpu_parity.py
KINDS = {"f32": ("single", False), "c64": ("single", True), "f64": ("double", False), "c128": ("double", True)}
GUARD = 4                                                     # elements before and after a buffer (16 / 32 bytes: the alignment stays)
CLS = {1: ndwt.nd_dwt_1D, 2: ndwt.nd_dwt_2D, 3: ndwt.nd_dwt_3D, 4: ndwt.nd_dwt_4D}

# LevelRouteKind of csrc/ndwt_select.h
FUSED3_DILATED, FUSED3, FUSED3_T, FUSED3_FOLD_T, FUSED2_DILATED, FUSED2, PER_AXIS = range(7)
# the longest fused tap length at tap stride 1 by (double, complex): 3-D (analysis, synthesis; the synthesis of float data beyond 16 /
# complex64 beyond 12 taps exists as Inv3Y only: even padding), 2-D (both ways)
FUSED3_MAX = {(False, False): (20, 20), (False, True): (16, 16), (True, False): (16, 16), (True, True): (12, 10)}
INV3Y_ONLY_FROM = {(False, False): 16, (False, True): 12}
FUSED2_MAX = {(False, False): 20, (False, True): 16, (True, False): 16, (True, True): 8}


def types(kind):
    prec, cplx = KINDS[kind]
    rdt = torch.float32 if prec == "single" else torch.float64
    ndt = (np.complex64 if prec == "single" else np.complex128) if cplx else (np.float32 if prec == "single" else np.float64)
    tdt = (torch.complex64 if prec == "single" else torch.complex128) if cplx else rdt
    return prec, cplx, rdt, ndt, tdt, ("float" if prec == "single" else "double"), TOL[prec]


# ------------------------------------------------------------------------------ which kernels a row must run (csrc/ndwt_select.h)
def padding_even(lens, Lp):
    return all(((Lp - n) // 2) % 2 == 0 for n in (list(lens) + [2, 2, 2])[:3])


def level_kind(row, kind, stride, inverse):
    """level_route of csrc/ndwt_select.h for the whole array: (LevelRouteKind, padded tap length)"""
    prec, cplx = KINDS[kind]
    f64, dims, lens, d = prec == "double", row["dims"], row["lens"], len(row["dims"])
    if row["generic"] or row["plan"] == "inter" or d == 1:
        return PER_AXIS, 0
    Lp = max(lens[:3])
    if d >= 3:
        fused1 = stride == 1 and Lp <= FUSED3_MAX[(f64, cplx)][inverse] and not (
            inverse and Lp > INV3Y_ONLY_FROM.get((f64, cplx), 99) and (not padding_even(lens, Lp) or row["vi"] in (3, 4)))
    else:
        fused1 = stride == 1 and Lp <= FUSED2_MAX[(f64, cplx)]
    if row["plan"] == "stack":                              # no sub-lattice form: a dilated level of a stack runs the per-axis passes
        return ((FUSED3 if d == 3 else FUSED2), Lp) if fused1 and d in (2, 3) else (PER_AXIS, 0)
    sub = not cplx and Lp <= 8 and (stride == 2 or (stride == 4 and not f64)) and all(n % stride == 0 for n in dims) and dims[0] % 4 == 0
    if d == 3 and sub:
        return FUSED3_DILATED, Lp
    if d >= 3 and fused1:
        return (FUSED3 if d == 3 else FUSED3_T), Lp
    if d == 2 and sub:
        return FUSED2_DILATED, Lp
    if d == 2 and fused1:
        return FUSED2, Lp
    return PER_AXIS, 0


def axis_specs(T, inverse):
    syn = "true" if inverse else "false"
    return [f"AxisMarch T={T} SYN={syn}", f"AxisX T={T} SYN={syn}", f"{'axis_synthesis_kernel' if inverse else 'axis_analysis_kernel'} T={T}"]


def expected(row, kind, inverse):
    """(must, may): every `must` spec is launched, and every launch is a `must` or a `may` spec.  A fused level names its kernel by
    family, scalar type, padded tap length and x step (EW = the tap stride of a dilated level, else the scalars per element); a level on
    the per-axis passes may run any of the three per-axis kernels of its direction -- which one is the selector's answer per pass
    (axis_select, csrc/ndwt_select.h; tests/test_dispatch_select.py checks it on the host, tests/test_gpu_dispatch.py against the
    trace), which this restatement does not repeat -- unless the row pins them (`axis`)."""
    prec, cplx = KINDS[kind]
    T, f64, comp = ("float" if prec == "single" else "double"), prec == "double", 2 if cplx else 1
    must, per_axis = [], False
    for lev in range(1, row["level"] + 1):
        stride = (1 << (lev - 1)) if row["dil"] == "atrous" else 1
        k, Lp = level_kind(row, kind, stride, inverse)
        if k == PER_AXIS:
            per_axis = True
            continue
        per_axis = per_axis or k == FUSED3_T                  # the t axis of a 4-D level is a per-axis pass
        dil = stride if k in (FUSED3_DILATED, FUSED2_DILATED) else 1
        ew = dil if dil > 1 else comp
        if k in (FUSED2, FUSED2_DILATED):
            assert row["dims"][1] < 64                          # (fused2_select: Inv2P from 64 rows on)
            s = f"{'Inv2S' if inverse else 'Fwd2S'} T={T} L={Lp} EW={ew}"
        elif not inverse:
            s = f"Fwd3 T={T} L={Lp} EW={ew}"
        else:
            # fused3_select: Inv3Y for float data with even padding (a level dilated by 4: 16-byte-aligned data only), else Inv3S
            vec4 = not row["offset"]
            y_ok = not f64 and Lp <= (20 if (dil > 1 or ew == 1) else 16) and row["vi"] not in (3, 4) and padding_even(row["lens"], Lp)
            use_y = y_ok and (dil == 1 or ((dil == 2 or (dil == 4 and vec4)) and row["vi"] != 2))
            s = f"{'Inv3Y' if use_y else 'Inv3S'} T={T} L={Lp} EW={ew}"
            if use_y and row["vi"] == 5:
                s += " DEPTH=1"
            if use_y and row["vi"] == 10 and (Lp == 8 or (ew == 4 and Lp in (4, 6))):   # the scatter form wherever it exists
                s += " XSC=true"
            if row["offset"] and dil > 1:
                s += " VEC4=false"
        if s not in must:
            must.append(s)
    if per_axis and row["axis"] is not None:
        return must + [f"{'axis_synthesis_kernel' if inverse else 'axis_analysis_kernel'} T={T}" if a == "element" else a for a in row["axis"]], []
    return must, axis_specs(T, inverse) if per_axis else []


def check(recs, must, may, what):
    """helpers.check_trace over the `must` specs and those `may` specs that something matched: nothing else may have run"""
    assert recs, f"{what}: nothing launched"
    used = [m for m in may if any(helpers.matches(r, helpers.spec(m)) for r in recs)]
    helpers.check_trace(recs, must + used, what)


# ------------------------------------------------------------------------------------------------------------------ rows
def R(rid, group, dims, wn, level, dil="atrous", plan="plain", K=1, inner=1, kinds=tuple(KINDS), vf=0, vi=0, generic=False, offset=False,
      axis=None, trace=True):
    wl = [wn] * len(dims) if isinstance(wn, str) else list(wn)
    assert len(wl) == len(dims) and all(2 * int(w[2:]) <= n for w, n in zip(wl, dims)), rid
    return dict(id=rid, group=group, dims=list(dims), wn=wl, lens=[2 * int(w[2:]) for w in wl], level=level, dil=dil, plan=plan, K=K, inner=inner,
                kinds=kinds, vf=vf, vi=vi, generic=generic, offset=offset, axis=axis, trace=trace)


REAL = ("f32", "f64")
ROWS = [
    # ---- a. fused sub-lattice routes shorter than the padded taps (real data: float strides 2 and 4, double stride 2; complex data and
    # double at stride 4 take the per-axis passes on the same shapes)
    R("a-8x8x8-db4-l1", "a", [8, 8, 8], "db4", 1),
    R("a-8x8x8-db4-l2", "a", [8, 8, 8], "db4", 2),
    R("a-8x8x8-db4-l3", "a", [8, 8, 8], "db4", 3),
    R("a-16x8x8-db4-l3", "a", [16, 8, 8], "db4", 3),
    R("a-12x8x8-db4-l3", "a", [12, 8, 8], "db4", 3),
    # (an axis of 4 takes at most db2: z sub-lattices of ONE sample under the 8 padded taps of x and y)
    R("a-8x8x4-db4.4.2-l3", "a", [8, 8, 4], ["db4", "db4", "db2"], 3),
    R("a-8x8x8-db2.4.2-l3", "a", [8, 8, 8], ["db2", "db4", "db2"], 3),
    R("a-8x4x4-db2-l3", "a", [8, 4, 4], "db2", 3),            # these three: no instance in the host emulation
    R("a-16x8x8-db3-l3", "a", [16, 8, 8], "db3", 3),
    R("a-4x4x4-db1-l3", "a", [4, 4, 4], "db1", 3),            # stride 4 = the axis: the level-3 details are identically zero
    R("a-2d-8x8-db4-l3", "a", [8, 8], "db4", 3),
    R("a-2d-16x4-db2-l3", "a", [16, 4], "db2", 3),
    R("a-2d-8x8-db4-l2", "a", [8, 8], "db4", 2, kinds=("f64", "f32")),
    R("a-8x8x8-db4-l3-inv4", "a", [8, 8, 8], "db4", 3, vi=4, kinds=REAL),
    R("a-8x8x8-db4-l3-inv5", "a", [8, 8, 8], "db4", 3, vi=5, kinds=REAL),
    R("a-8x8x8-db4-l3-inv10", "a", [8, 8, 8], "db4", 3, vi=10, kinds=REAL),
    R("a-16x8x8-db3-l3-inv4", "a", [16, 8, 8], "db3", 3, vi=4, kinds=("f32",)),
    R("a-16x8x8-db3-l3-inv5", "a", [16, 8, 8], "db3", 3, vi=5, kinds=("f32",)),
    R("a-16x8x8-db3-l3-inv10", "a", [16, 8, 8], "db3", 3, vi=10, kinds=("f32",)),
    R("a-8x4x4-db2-l3-inv5", "a", [8, 4, 4], "db2", 3, vi=5, kinds=("f32",)),
    R("a-8x4x4-db2-l3-inv10", "a", [8, 4, 4], "db2", 3, vi=10, kinds=("f32",)),
    R("a-4x4x4-db1-l3-inv4", "a", [4, 4, 4], "db1", 3, vi=4, kinds=("f32",)),
    R("a-4x4x4-db1-l3-inv5", "a", [4, 4, 4], "db1", 3, vi=5, kinds=("f32",)),
    R("a-8x8x4-db4.4.2-l3-inv4", "a", [8, 8, 4], ["db4", "db4", "db2"], 3, vi=4, kinds=("f32",)),
    R("a-8x8x8-db4-l3-offset", "a", [8, 8, 8], "db4", 3, offset=True, kinds=REAL),
    # ---- b. per-axis routes
    R("b-10x9x7-db3.2.2-l3", "b", [10, 9, 7], ["db3", "db2", "db2"], 3, axis=["element"]),     # 10 / 2 = 5 < 6 taps, 9 and 7 odd: no AxisMarch
    R("b-2d-9x6-db2.3-l3", "b", [9, 6], ["db2", "db3"], 3),
    R("b-1d-10-db5-l4", "b", [10], "db5", 4, axis=["element"]),
    # (an axis of 8 takes at most db4) every axis divides by 2 and 4, n / stride < L everywhere: AxisMarch refused, the element kernels run
    # (complex128 has no fused 12-tap synthesis: its level 1 at tap stride 1 may march, so it is left to the rows above and below)
    R("b-16x16x8-db6.6.4-l3", "b", [16, 16, 8], ["db6", "db6", "db4"], 3, axis=["element"], kinds=("f32", "f64", "c64")),
    R("b-8x6x4-db3.2.2-l3", "b", [8, 6, 4], ["db3", "db2", "db2"], 3, kinds=("c64", "c128")),
    R("b-4d-6x4x5x4-l3", "b", [6, 4, 5, 4], ["db3", "db2", "db2", "db1"], 3),
    R("b-1d-8-db4-l5", "b", [8], "db4", 5, axis=["element"]),   # strides 8 and 16: the details of levels 4 and 5 are identically zero
    R("b-1d-6-db3-l4", "b", [6], "db3", 4, axis=["element"]),   # stride 8 = 2 mod 6
    R("b-8x8x8-db4-l3-generic", "b", [8, 8, 8], "db4", 3, generic=True),
    # ---- c. the newer plan kinds
    R("c-batch-8x3-db4-l3", "c", [8], "db4", 3, plan="many", K=3, axis=["element"]),
    R("c-stack2-8x8x3-db4-l3", "c", [8, 8], "db4", 3, plan="stack", K=3),
    R("c-stack3-8x8x4x2-l3", "c", [8, 8, 4], ["db4", "db4", "db2"], 3, plan="stack", K=2),
    R("c-inter-4x8x2-db4-l3", "c", [8], "db4", 3, plan="inter", inner=4, K=2),
    R("c-inter-3x6x5-db3.2-l3", "c", [6, 5], ["db3", "db2"], 3, plan="inter", inner=3, K=1),
    # ---- d. the reference's dilation at the shortest legal axes
    *[R(f"d-{n}d-n{2 * o}-db{o}", "d", [2 * o] * n, f"db{o}", 3, dil="reference") for n in (3, 2, 1) for o in range(1, 11)],
    R("d-2x20x4-db1.10.2", "d", [2, 20, 4], ["db1", "db10", "db2"], 3, dil="reference"),       # an axis of 2 under 20 padded taps wraps ten times
    R("d-2d-20x2-db10.1", "d", [20, 2], ["db10", "db1"], 3, dil="reference"),
    R("d-4x2x12-db2.1.6", "d", [4, 2, 12], ["db2", "db1", "db6"], 3, dil="reference"),
    # AxisX takes rows of n * comp >= 8 L scalars (axis_select): one side, the threshold, the other side -- for real and complex data
    *[R(f"d-1d-n{n}-db{o}", "d", [n], f"db{o}", 3, dil="reference", kinds=kinds)
      for o in (2, 6) for m, kinds in ((16 * o, REAL), (8 * o, ("c64", "c128"))) for n in (m - 1, m, m + 1)],
    # variant 11 / 11 (the cascades wherever they exist): whatever runs, the values hold
    *[R(f"d-2d-n{2 * o}-db{o}-v11", "d", [2 * o] * 2, f"db{o}", 3, dil="reference", vf=11, vi=11, trace=False) for o in (1, 2, 4, 6, 10)],
    *[R(f"d-batch-n{n}x3-db{o}-v{v}", "d", [n], f"db{o}", 3, dil="reference", plan="many", K=3, vf=v, vi=v, trace=False)
      for o in (2, 4) for n in (2 * o, 16 * o) for v in (0, 11)],
]
IDS = [r["id"] for r in ROWS]
assert len(set(IDS)) == len(IDS)


# --------------------------------------------------------------------------------------------------------- data and oracle
class Buf:
    """n elements with GUARD zero elements before and after (off: where the buffer starts inside the allocation)"""

    def __init__(self, n, tdt, off=GUARD, fill=None):
        self.t = torch.zeros(n + off + GUARD, dtype=tdt, device="cuda")
        self.off, self.n, self.view = off, n, self.t[off:off + n]
        if fill is not None:
            self.view.fill_(fill)

    def ptr(self):
        return self.view.data_ptr()

    def clean_outside(self):
        return float(self.t[:self.off].abs().sum()) == 0 and float(self.t[self.off + self.n:].abs().sum()) == 0


def stream():
    return torch.cuda.current_stream().cuda_stream


def whole_shape(row):
    """the whole array in MATLAB order (first index fastest), and the filtered axes in it"""
    d = len(row["dims"])
    if row["plan"] == "plain":
        return tuple(row["dims"]), tuple(range(d))
    if row["plan"] in ("many", "stack"):
        return tuple(row["dims"]) + (row["K"],), tuple(range(d))
    return (row["inner"],) + tuple(row["dims"]) + (row["K"],), tuple(range(1, d + 1))


def make_plan(row, kind):
    prec, cplx, rdt = types(kind)[:3]
    dims, wl, l2, dil, lev = row["dims"], row["wn"], row["l2"], row["dil"], row["level"]
    if row["plan"] == "many":
        p = ndwt.Plan(dims, wl, rdt, cplx, l2, dil, max_level=lev, howmany=row["K"])
    elif row["plan"] == "stack":
        p = ndwt.Plan(dims + [row["K"]], wl + [None], rdt, cplx, l2, dil, max_level=lev, axes=tuple(range(len(dims))))
    elif row["plan"] == "inter":
        p = ndwt.Plan(dims, wl, rdt, cplx, l2, dil, max_level=lev, inner=row["inner"], howmany=row["K"])
    else:
        p = ndwt.Plan(dims, wl, rdt, cplx, l2, dil, max_level=lev)
    if row["vf"] or row["vi"]:
        p.set_variant(fwd=row["vf"], inv=row["vi"])
    if row["generic"]:
        p.set_path(True)
    return p


def per_item(fn, a, axes, extra=0):
    """fn over the filtered axes `axes` of `a` (whose last `extra` axes belong to the items too: the bands), item by item"""
    lead = [k for k in range(a.ndim - extra) if k not in axes]
    b = np.moveaxis(a, lead, range(len(lead)))
    out = None
    for idx in np.ndindex(*b.shape[:len(lead)]):
        r = fn(b[idx])
        if out is None:
            out = np.zeros(b.shape[:len(lead)] + r.shape, dtype=r.dtype)
        out[idx] = r
    return np.moveaxis(out, range(len(lead)), lead)


def oracle_dec(row, x, axes):
    return per_item(lambda v: orc.spatial_dec(v, row["wn"], row["level"], row["l2"], row["dil"]), x, axes)


def oracle_rec(row, c, axes):
    return per_item(lambda v: orc.spatial_rec(v, row["wn"], row["l2"], row["dil"], level=row["level"]), c, axes, extra=1)


def randn(rng, shape, kind):
    prec, cplx, rdt, ndt = types(kind)[:4]
    a = rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if cplx else 0)
    return a.astype(ndt).astype(np.complex128 if cplx else np.float64)      # what the device gets, exactly


def to_dev(a, kind, off=GUARD):
    ndt, tdt = types(kind)[3], types(kind)[4]
    b = Buf(a.size, tdt, off)
    b.view.copy_(torch.from_numpy(np.ascontiguousarray(np.transpose(a)).astype(ndt).reshape(-1)).cuda())
    return b


def from_dev(b, shape):
    return np.transpose(b.view.cpu().numpy().reshape(tuple(reversed(shape))))


def dec_error(got, want, x, zero):
    """relative to max|want| over the bands that are not identically zero; those: max|got| against max|x|"""
    err = np.abs(got[..., ~zero] - want[..., ~zero]).max() / np.abs(want[..., ~zero]).max()
    if zero.any():
        err = max(err, np.abs(got[..., zero]).max() / np.abs(x).max())
    return float(err)


WORST = {}


def note(row, kind, what, err, bound):
    """the figures of a row, printed before they are asserted; the worst ratio per group is printed as the group goes on"""
    g = WORST.setdefault(row["group"], {})
    if err / bound >= g.get(what, (0, 0, 0))[0]:
        g[what] = (err / bound, err, f"{row['id']} {kind} l2={row['l2']}")
    print(f"[short-axes {row['group']}] {row['id']} {kind} l2={row['l2']} {what}: {err:.3g} (bound {bound:.3g}); "
          f"worst of the group so far {g[what][1]:.3g} = {g[what][0]:.3f} of its bound ({g[what][2]})")


def run_transforms(row, kind):
    """dec, rec of random coefficients, rec(dec(x)): values, traces, guard elements.  Returns (plan, x, the oracle's coefficients)"""
    prec, cplx, rdt, ndt, tdt, T, tol = types(kind)
    shape, axes = whole_shape(row)
    nb = orc.num_bands(len(axes), row["level"])
    rng = np.random.default_rng(zlib.crc32(repr((row["id"], kind, row["l2"])).encode()))
    x = randn(rng, shape, kind)
    c = randn(rng, shape + (nb,), kind)
    want_y, want_r = oracle_dec(row, x, axes), oracle_rec(row, c, axes)
    zero = helpers.zero_bands(row["dims"], row["level"], row["dil"])
    assert not zero.any() or np.abs(want_y[..., zero]).max() <= 1e-12 * np.abs(x).max()     # the oracle agrees that they are zero
    p = make_plan(row, kind)
    off = GUARD + 1 if row["offset"] else GUARD               # (offset: every pointer one element off the 16-byte grid)
    what = f"{row['id']} {kind} l2={row['l2']}"
    xb, yb = to_dev(x, kind, off), Buf(x.size * nb, tdt, off, float("nan"))
    with ndwt.kernel_trace() as recs_d:
        p.dec(xb.ptr(), yb.ptr(), row["level"], stream())
    cb, rb = to_dev(c, kind, off), Buf(x.size, tdt, off, float("nan"))
    with ndwt.kernel_trace() as recs_r:
        p.rec(cb.ptr(), rb.ptr(), row["level"], stream())
    tb = Buf(x.size, tdt, off, float("nan"))
    with ndwt.kernel_trace() as recs_t:
        p.rec(yb.ptr(), tb.ptr(), row["level"], stream())
    torch.cuda.synchronize()
    got_y, got_r, got_t = from_dev(yb, shape + (nb,)), from_dev(rb, shape), from_dev(tb, shape)
    assert np.isfinite(got_y).all() and np.isfinite(got_r).all() and np.isfinite(got_t).all(), f"{what}: an output element was not written"
    e_dec = dec_error(got_y, want_y, x, zero)
    e_rec = float(np.abs(got_r - want_r).max() / np.abs(want_r).max())
    e_rt = float(np.abs(got_t - x).max() / np.abs(x).max())
    note(row, kind, "dec", e_dec, tol)
    note(row, kind, "rec", e_rec, 4 * tol)
    note(row, kind, "rec(dec)", e_rt, 20 * tol)
    print(f"    dec ran {sorted({repr(r).split(' grid')[0] for r in recs_d})}\n    rec ran {sorted({repr(r).split(' grid')[0] for r in recs_r})}")
    assert e_dec <= tol, (what, "dec", e_dec)
    assert e_rec <= 4 * tol, (what, "rec", e_rec)
    assert e_rt <= 20 * tol, (what, "rec(dec)", e_rt)
    for b in (xb, yb, cb, rb, tb):
        assert b.clean_outside(), f"{what}: wrote outside a buffer"
    if row["trace"]:
        check(recs_d, *expected(row, kind, False), f"{what} dec")
        for recs in (recs_r, recs_t):
            check(recs, *expected(row, kind, True), f"{what} rec")
    else:
        assert recs_d and recs_r and recs_t, f"{what}: nothing launched"
    return p, x, want_y, xb


CASES = [pytest.param(row, kind, id=f"{row['id']}-{kind}") for row in ROWS if row["group"] != "c" for kind in row["kinds"]]


@pytest.mark.parametrize("row,kind", CASES)
def test_short_axes_against_the_oracle(row, kind):
    for l2 in (0, 1):
        run_transforms(dict(row, l2=l2), kind)


def test_generic_path_equals_the_auto_path_on_a_wrapping_shape():
    """NDWT_PATH_GENERIC on [8, 8, 8] db4 a-trous at 3 levels: the auto path (sub-lattice kernels) within 4 TOL of it, both ways"""
    auto, gen = next(r for r in ROWS if r["id"] == "a-8x8x8-db4-l3"), next(r for r in ROWS if r["id"] == "b-8x8x8-db4-l3-generic")
    for kind in REAL:
        prec, cplx, rdt, ndt, tdt, T, tol = types(kind)
        for l2 in (0, 1):
            rng = np.random.default_rng(88 + l2)
            x, c = randn(rng, (8, 8, 8), kind), randn(rng, (8, 8, 8, 22), kind)
            xb, cb, out = to_dev(x, kind), to_dev(c, kind), {}
            for name, row in (("auto", auto), ("generic", gen)):
                p = make_plan(dict(row, l2=l2), kind)
                yb, rb = Buf(x.size * 22, tdt, GUARD, float("nan")), Buf(x.size, tdt, GUARD, float("nan"))
                with ndwt.kernel_trace() as recs:
                    p.dec(xb.ptr(), yb.ptr(), 3, stream())
                    p.rec(cb.ptr(), rb.ptr(), 3, stream())
                torch.cuda.synchronize()
                fused = {r.family for r in recs} & {"Fwd3", "Inv3Y", "Inv3S"}
                assert bool(fused) == (name == "auto"), (name, recs)
                out[name] = (from_dev(yb, (8, 8, 8, 22)), from_dev(rb, (8, 8, 8)))
            e_dec = float(np.abs(out["auto"][0] - out["generic"][0]).max() / np.abs(out["generic"][0]).max())
            e_rec = float(np.abs(out["auto"][1] - out["generic"][1]).max() / np.abs(out["generic"][1]).max())
            print(f"[short-axes b] generic against auto, {kind} l2={l2}: dec {e_dec:.3g}, rec {e_rec:.3g} (bound {4 * tol:.3g})")
            assert e_dec <= 4 * tol and e_rec <= 4 * tol, (kind, l2, e_dec, e_rec)


# ------------------------------------------------------------------------------------------- c. denoise on the newer plan kinds
def np_shrink_bands(c, thr, hard):
    """band b of c[..., b] shrunk by thr[b] (complex: the magnitude); 0 leaves the band as it is"""
    out = c.copy()
    for b, t in enumerate(thr):
        if t == 0:
            continue
        m = np.abs(c[..., b])
        out[..., b] = c[..., b] * (np.where(m > t, 1.0, 0.0) if hard else np.where(m > t, (m - t) / np.where(m > 0, m, 1.0), 0.0))
    return out


def gap_thresholds(c, tol, zero):
    """hard mode: per detail band the middle of the widest gap of the oracle's sorted |c| of that band; the gap is at least
    200 tol max|c|, so that no coefficient is within rounding of its threshold (and none is masked out of the comparison).  Band 0 and
    the bands that are identically zero (rounding noise on both sides) get 0 = left as they are."""
    thr = np.zeros(c.shape[-1])
    for b in range(1, c.shape[-1]):
        if zero[b]:
            continue
        m = np.sort(np.abs(c[..., b]).reshape(-1))
        gaps = np.diff(m)
        i = int(np.argmax(gaps))
        assert gaps[i] >= 200 * tol * np.abs(c).max(), f"band {b}: widest gap {gaps[i]:.3g} < {200 * tol * np.abs(c).max():.3g}: choose another seed"
        thr[b] = 0.5 * (m[i] + m[i + 1])
    return thr


CASES_C = [pytest.param(row, kind, id=f"{row['id']}-{kind}") for row in ROWS if row["group"] == "c" for kind in row["kinds"]]


@pytest.mark.parametrize("row,kind", CASES_C)
def test_newer_plan_kinds_short_and_atrous(row, kind):
    prec, cplx, rdt, ndt, tdt, T, tol = types(kind)
    for l2 in (0, 1):
        row = dict(row, l2=l2)
        p, x, c, xb = run_transforms(row, kind)
        shape, axes = whole_shape(row)
        zero = helpers.zero_bands(row["dims"], row["level"], row["dil"])
        for hard in (False, True):
            if hard:
                thr = gap_thresholds(c, tol, zero)
            else:
                thr = 1.5 * ndwt.band_gains(row["dims"], row["wn"], row["level"], pres_l2_norm=l2, dilation=row["dil"])
                thr[0] = 0.0
            want = oracle_rec(row, np_shrink_bands(c, thr, hard), axes)
            ob = Buf(x.size, tdt, GUARD, float("nan"))
            with ndwt.kernel_trace() as recs:
                p.denoise_bands(xb.ptr(), ob.ptr(), row["level"], thr, hard, stream())
            torch.cuda.synchronize()
            got = from_dev(ob, shape)
            what = f"{row['id']} {kind} l2={l2} denoise {'hard' if hard else 'soft'}"
            assert np.isfinite(got).all(), f"{what}: an element of out was not written"
            err = float(np.abs(got - want).max() / max(np.abs(want).max(), 1.0))
            note(row, kind, "denoise hard" if hard else "denoise soft", err, 20 * tol)
            assert err <= 20 * tol, (what, err)
            assert ob.clean_outside() and xb.clean_outside(), f"{what}: wrote outside a buffer"
            (md, yd), (mr, yr) = expected(row, kind, False), expected(row, kind, True)
            assert sum(r.family == "shrink_kernel" for r in recs) == int(np.count_nonzero(thr)), f"{what}: one shrink pass per non-zero band: {recs}"
            check(recs, md + [m for m in mr if m not in md] + [f"shrink_kernel T={T} COMP={2 if cplx else 1}"], yd + yr, what)


# ------------------------------------------------------------------------------------------- the generator, through the classes
SHORT = helpers.short_axis_cases(48, seed=20261019)


@pytest.mark.parametrize("case", SHORT, ids=[helpers.fuzz_id(c) for c in SHORT])
def test_short_axis_cases_through_the_classes(case):
    """fixed-seed subset of helpers.short_axis_cases (tools/fuzz_gpu.py .. short) through nd_dwt_1D .. 4D: dec, rec of arbitrary
    coefficients, round trip"""
    d, sizes, wn, level, l2 = case["d"], case["sizes"], case["wn"], case["level"], case["l2"]
    precision, cplx, dilation = case["precision"], case["cplx"], case["dilation"]
    kind = {("single", False): "f32", ("single", True): "c64", ("double", False): "f64", ("double", True): "c128"}[(precision, cplx)]
    tdt, tol = types(kind)[4], TOL[precision]
    row = dict(id=helpers.fuzz_id(case), group="fuzz", l2=l2)
    rng = np.random.default_rng(case["data_seed"])
    x = randn(rng, sizes, kind)
    w = CLS[d](wn if d > 1 else wn[0], sizes, "pres_l2_norm", l2, "precision", precision, "dilation", dilation)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(np.transpose(a))).cuda().to(tdt).permute(*reversed(range(a.ndim)))   # noqa: E731
    xg = dev(x)
    with ndwt.kernel_trace() as recs:
        y = w.dec(xg, level)
        r = w.rec(y)
    assert recs
    want = orc.spatial_dec(x, wn, level, l2, dilation)
    zero = helpers.zero_bands(sizes, level, dilation)
    e_dec = dec_error(y.cpu().numpy(), want, x, zero)
    e_rt = float(np.abs(r.cpu().numpy() - x).max() / np.abs(x).max())
    c = randn(rng, want.shape, kind)
    want_r = orc.spatial_rec(c, wn, l2, dilation, level=level)
    e_rec = float(np.abs(w.rec(dev(c)).cpu().numpy() - want_r).max() / np.abs(want_r).max())
    note(row, kind, "dec", e_dec, tol)
    note(row, kind, "rec", e_rec, 4 * tol)
    note(row, kind, "rec(dec)", e_rt, 20 * tol)
    assert e_dec <= tol and e_rec <= 4 * tol and e_rt <= 20 * tol, (e_dec, e_rec, e_rt)
