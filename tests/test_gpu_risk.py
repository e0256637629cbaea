"""The SURE statistics and thresholds on the device: ndwt_band_risk, ndwt_band_risk_items, ndwt_sure_thresholds(_items) and the classes'
band_risk and sure_thresholds.

The statistics need no transform: the coefficient array is ARBITRARY DATA written by the test (tests/norms_cases.py: an all-equal item,
an item with a NaN, an all-zero item with one -0, integer-valued items), the plan only supplies the sizes, the items and the data kind.
Every array lies between guard words, the bands on a pitch have guard words between them, and the whole buffer is compared with its copy
afterwards.  The shapes are those of tests/test_gpu_norms.py, the smallest at which each form of the kernel can go wrong:

  1-D, n = 37, db2, float, level 2                      element-wise, below one workgroup
  batch 5 x 96, db2, complex64, level 3                 the 4-scalar form, 4 bands x 5 items
  batch 2 x 20000, db4, float and double, level 1       chunks > 1 with a ragged last chunk, so RiskFinish runs; once more with
                                                        set_tuning(target_blocks=1): one chunk and one launch
  stack 8 x 12 x 3 items, db2, complex128, level 2      7 bands, band_pitch = ndwt_band_pitch, guard words between and behind the bands
  3-D 8 x 8 x 8, db2, double, level 2                   15 bands; the array one element off a 32-byte boundary: the element-wise form
  interleaved, inner = 3, 15 x 15, db1, float, level 1  the items of ndwt_plan_create_interleaved: 675 scalars, no multiple of 4

  values     nc = 8, 3 and 1 against numpy on the host copy with the candidates, the tolerances and the exact cases of tests/risk_cases.py
             (derived there); one block's row begins with a negative entry: zeros
  trace      chunks = 1: exactly one BandRisk record; chunks > 1: one BandRisk and one RiskFinish, with the grids norms_chunks gives
  norms      COUNT at t = 0 is elements - nnz of band_norms (blocks without a NaN); COUNT at +inf is the elements and ENERGY there is
             l2sq within n 2^-52 (each is within (n - 1) 2^-53 of the exact sum)
  pooled     the pooled call against the per-item rows at the same candidates: the counts add exactly
  shrink     real data: after shrink_bands(hard) with column i of the candidates the zeros of every band number COUNT[i]
  select     complex data: COUNT at the k-th order statistic of band_select is k + 1 where the k-th and the (k + 1)-th differ
  search     sure_thresholds(_items) on dec of a piecewise signal plus seeded noise against the numpy restatement of the search fed with
             numpy statistics: equal to 1e-12 relative, or, where they differ, numpy's estimate at the returned threshold within
             1e-9 n d s^2 of numpy's pick (a tie; 1e-9 is far above the n 2^-53 summation error); per item with one item of noise alone;
             rounds = 1 against 3; band 0 is 0; denoise accepts the row; the classes' hybrid branch
  refusals   name the argument and launch nothing
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import ndwt_amd as ndwt
from items_cases import build_named_shim
from norms_cases import L2SQ, NNZ, norms_array
from risk_cases import COUNT, ENERGY, INVSUM, blocks_of, candidate_row, check_block, reference, search, sure
from select_cases import KINDS

pytestmark = pytest.mark.gpu

GUARD = 8                                                     # scalars before and after an array (32 / 64 bytes: the alignment stays)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = build_named_shim(tmp_path_factory, "norms_shim")
    lib.sel_norms_chunks.argtypes = [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_int]
    lib.sel_norms_chunks.restype = ctypes.c_longlong
    return lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def torch_real(kind):
    return torch.float32 if KINDS[kind][0] == np.float32 else torch.float64


def tname(kind):
    return "float" if KINDS[kind][0] == np.float32 else "double"


# id -> (plan, items, elements of one item, filtered axes, level, pitched, skew in elements, the 4-scalar form)
def make_case(kind, shape):
    rdt, cplx = torch_real(kind), KINDS[kind][1]
    if shape == "1d-37":
        return ndwt.Plan([37], ["db2"], rdt, cplx, max_level=2), 1, 37, 1, 2, False, 0, False
    if shape == "batch-5x96":
        return ndwt.Plan([96], ["db2"], rdt, cplx, max_level=3, howmany=5), 5, 96, 1, 3, False, 0, True
    if shape == "batch-2x20000":
        return ndwt.Plan([20000], ["db4"], rdt, cplx, max_level=1, howmany=2), 2, 20000, 1, 1, False, 0, True
    if shape == "stack-3x8x12":
        return ndwt.Plan([8, 12, 3], ["db2", "db2", None], rdt, cplx, max_level=2, axes=(0, 1)), 3, 96, 2, 2, True, 0, True
    if shape == "3d-8x8x8-skew":
        return ndwt.Plan([8, 8, 8], ["db2"] * 3, rdt, cplx, max_level=2), 1, 512, 3, 2, False, 1, False
    if shape == "inner-3-15x15":
        return ndwt.Plan([15, 15], ["db1", "db1"], rdt, cplx, max_level=1, inner=3, howmany=2), 2, 675, 2, 1, False, 0, False
    raise ValueError(shape)


CASES = [("f32", "1d-37"), ("c64", "batch-5x96"), ("f32", "batch-2x20000"), ("f64", "batch-2x20000"), ("c128", "stack-3x8x12"),
         ("f64", "3d-8x8x8-skew"), ("f32", "inner-3-15x15")]


class Coefs:
    """a coefficient array of tests/norms_cases.py between GUARD scalars of filler (and `skew` elements further), on the device, with its
    host copy"""

    def __init__(self, kind, items, N, nb, pitch_elements, seed, skew=0):
        rdt, cplx = KINDS[kind]
        self.comp = 2 if cplx else 1
        n = items * N * self.comp
        self.bs = (pitch_elements or items * N) * self.comp
        self.flat, pitch, self.integer = norms_array(kind, items, N, nb, self.bs - n, seed)
        assert pitch == self.bs
        self.off = GUARD + skew * self.comp
        self.host = np.full(self.off + nb * self.bs + GUARD, 1e30, dtype=rdt)
        self.host[self.off:self.off + nb * self.bs] = self.flat
        self.dev = torch.from_numpy(self.host).cuda()
        self.ptr = self.dev.data_ptr() + self.off * self.host.itemsize

    def unchanged(self):
        return self.dev.cpu().numpy().tobytes() == self.host.tobytes()


def same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.mark.parametrize("kind,shape", CASES, ids=[f"{k}-{s}" for k, s in CASES])
def test_the_statistics_of_every_block(shim, kind, shape):
    rdt, cplx = KINDS[kind]
    plan, items, N, axes, level, pitched, skew, vec = make_case(kind, shape)
    comp = 2 if cplx else 1
    assert plan.items == items
    nb = ndwt.num_bands(axes, level)
    pitch = plan.band_pitch() if pitched else 0
    seed = zlib.crc32(f"{kind}-{shape}".encode()) % 100000
    c = Coefs(kind, items, N, nb, pitch, seed, skew)
    n = N * comp

    def is_vec(n_scalars):
        return c.ptr % (4 * c.host.itemsize) == 0 and c.bs % 4 == 0 and n_scalars % 4 == 0
    assert vec == is_vec(n)
    fam = {"T": tname(kind), "COMP": comp}

    def traced(f, n_scalars, n_items, target=0):
        """f() with its trace checked: one BandRisk on bands x items x chunks workgroups, and one RiskFinish where chunks > 1"""
        v = is_vec(n_scalars)
        chunks = int(shim.sel_norms_chunks(n_scalars, comp, int(v), nb, n_items, cus(), target))
        with ndwt.kernel_trace() as recs:
            out = f()
        assert len(recs) == (1 if chunks == 1 else 2), recs
        assert recs[0].family == "BandRisk" and recs[0].params == dict(fam, VEC=v), recs[0]
        assert recs[0].grid == (nb * n_items * chunks, 1, 1) and recs[0].block == (256, 1, 1), (recs[0], chunks)
        if chunks > 1:
            assert recs[1].family == "RiskFinish" and recs[1].grid == (nb * n_items, 1, 1) and recs[1].block == (64, 1, 1), recs[1]
        return out, chunks

    # -- per item: nc = 8, 3 and 1, a row of its own for every block; the row of (band 0, item 0) skips its block
    per8 = None
    for nc in (8, 3, 1):
        cand = np.zeros((items, nb, nc))
        for b, j, blk in blocks_of(kind, c.flat, c.bs, items, N, nb):
            cand[j, b] = candidate_row(kind, blk, nc, vec, seed + 31 * b + j)
        cand[0, 0, 0] = -1.0
        got, chunks = traced(lambda: plan.band_risk_items(c.ptr, level, cand, stream(), band_pitch=pitch), n, items)
        assert got.shape == (items, nb, nc, 3)
        assert chunks == (2 if shape == "batch-2x20000" else 1)     # 5000 steps: two chunks, the last one ragged
        for b, j, blk in blocks_of(kind, c.flat, c.bs, items, N, nb):
            check_block(kind, blk, cand[j, b], got[j, b], vec, (b, j) in c.integer, f"{kind}-{shape} nc {nc} band {b} item {j}")
        assert not got[0, 0].any()
        assert same(plan.band_risk_items(c.ptr, level, cand, stream(), band_pitch=pitch), got)   # a fixed order: the same bits
        if nc == 8:
            per8, cand8 = got, cand
    if shape == "batch-2x20000":
        # one chunk and one launch on request: the same counts, the sums within their bound (another order)
        plan.set_tuning(target_blocks=1)
        one, ch = traced(lambda: plan.band_risk_items(c.ptr, level, cand8, stream(), band_pitch=pitch), n, items, 1)
        assert ch == 1
        for b, j, blk in blocks_of(kind, c.flat, c.bs, items, N, nb):
            check_block(kind, blk, cand8[j, b], one[j, b], vec, (b, j) in c.integer, f"{kind}-{shape} one chunk band {b} item {j}")
        assert same(one[..., COUNT], per8[..., COUNT])
        plan.set_tuning(target_blocks=0)
        assert same(plan.band_risk_items(c.ptr, level, cand8, stream(), band_pitch=pitch), per8)

    # -- pooled: the band is the whole array; against numpy, and against the per-item rows at the same candidates
    pvec = is_vec(items * n)
    shared = np.zeros((nb, 8))
    for b in range(nb):
        shared[b] = candidate_row(kind, c.flat[b * c.bs:b * c.bs + items * n], 8, pvec, seed + b)
    pooled, _ = traced(lambda: plan.band_risk(c.ptr, level, shared, stream(), band_pitch=pitch), items * n, 1)
    assert pooled.shape == (nb, 8, 3)
    for b in range(nb):
        check_block(kind, c.flat[b * c.bs:b * c.bs + items * n], shared[b], pooled[b], pvec, all((b, j) in c.integer for j in range(items)),
                    f"{kind}-{shape} pooled band {b}")
    rows = plan.band_risk_items(c.ptr, level, np.broadcast_to(shared, (items, nb, 8)), stream(), band_pitch=pitch)
    if items == 1:
        assert same(rows[0], pooled)                              # one item: the per-item call equals the pooled one
    if pvec == vec or kind != "c64":                              # (the two float forms of the complex magnitude round differently)
        assert np.array_equal(pooled[..., COUNT], rows[..., COUNT].sum(axis=0))
        want = rows[..., ENERGY].sum(axis=0)
        ok = np.abs(pooled[..., ENERGY] - want) <= items * n * 2.0 ** -52 * np.abs(want)
        assert (ok | (np.isnan(want) & np.isnan(pooled[..., ENERGY]))).all()

    # -- against band_norms: t = 0 and t = +inf
    ends = np.zeros((items, nb, 2))
    ends[..., 1] = np.inf
    got = plan.band_risk_items(c.ptr, level, ends, stream(), band_pitch=pitch)
    norms = plan.band_norms_items(c.ptr, level, stream(), band_pitch=pitch)
    assert (got[..., 1, COUNT] == N).all() and not got[..., 1, INVSUM].any()
    for b, j, blk in blocks_of(kind, c.flat, c.bs, items, N, nb):
        if np.isnan(blk).any():
            assert np.isnan(got[j, b, 1, ENERGY]) and np.isnan(norms[j, b, L2SQ])
            continue
        assert got[j, b, 0, COUNT] == N - norms[j, b, NNZ], (b, j)
        assert abs(got[j, b, 1, ENERGY] - norms[j, b, L2SQ]) <= n * 2.0 ** -52 * norms[j, b, L2SQ], (b, j)
    assert c.unchanged()                                          # the array, the guard words between and around the bands


def test_after_a_hard_shrink_the_zeros_of_every_band_number_the_count():
    plan = ndwt.Plan([96], ["db2"], torch.float32, False, max_level=3, howmany=5)
    items, N, level, nb = 5, 96, 3, 4
    rng = np.random.default_rng(17)
    host = rng.standard_normal(nb * items * N).astype(np.float32)
    host[::7] = 0.0                                               # zeros of its own: what a threshold of 0 counts
    cand = np.array([[0.0, 0.3, 1.1], [0.5, float(np.abs(host[items * N + 5])), 0.0], [0.0, 2.0, 0.7], [1.25, np.inf, 0.1]])
    y = torch.from_numpy(host).cuda()
    got = plan.band_risk(y.data_ptr(), level, cand, stream())
    assert same(y.cpu().numpy(), host)
    for i in range(3):
        z = torch.from_numpy(host).cuda()
        thr = np.where(np.isinf(cand[:, i]), 1e30, cand[:, i])   # (the shrink takes finite thresholds; nothing here is above 1e30)
        plan.shrink_bands(z.data_ptr(), level, thr, True, stream())
        zeros = (z.cpu().numpy().reshape(nb, items * N) == 0).sum(axis=1)
        assert np.array_equal(zeros, got[:, i, COUNT]), (i, zeros, got[:, i, COUNT])


def test_the_count_at_an_order_statistic_of_complex_data_is_its_rank_plus_one():
    plan = ndwt.Plan([96], ["db2"], torch.float32, True, max_level=3, howmany=5)
    items, N, level, nb = 5, 96, 3, 4
    rng = np.random.default_rng(29)
    host = rng.standard_normal(nb * items * N * 2).astype(np.float32)
    y = torch.from_numpy(host).cuda()
    E = items * N
    ks = [E // 3, E // 3 + 1, E - 2, E - 1]
    cand = np.zeros((nb, 2))
    vals = np.zeros((nb, 4))
    for b in range(nb):
        vals[b] = plan.band_select(y.data_ptr(), level, b, ks, stream())
        cand[b] = [vals[b, 0], vals[b, 2]]
    got = plan.band_risk(y.data_ptr(), level, cand, stream())
    checked = 0
    for b in range(nb):
        for col, k in ((0, 0), (1, 2)):
            if vals[b, k] != vals[b, k + 1]:
                assert got[b, col, COUNT] == ks[k] + 1, (b, ks[k], got[b, col])
                checked += 1
    assert checked >= nb                                          # (continuous data: ties are the exception)
    top = np.array([[plan.band_select(y.data_ptr(), level, b, [E - 1], stream())[0]] for b in range(nb)])
    at_top = plan.band_risk(y.data_ptr(), level, top, stream())
    assert (at_top[:, 0, COUNT] == E).all() and not at_top[:, 0, INVSUM].any()   # nothing lies above the largest magnitude


def piecewise(n):
    t = np.arange(n)
    return np.where(t < n // 3, 2.0, -1.0) + np.where(t % 200 < 70, 1.5, 0.0) + np.where(t > 3 * n // 4, 0.01 * (t - 3 * n // 4), 0.0)


@pytest.mark.parametrize("kind", ["f64", "c64"])
def test_the_search_is_its_numpy_restatement(kind):
    rdt, cplx = KINDS[kind]
    comp = 2 if cplx else 1
    K, N, level, sigma = 3, 1024, 3, 0.3
    nb = ndwt.num_bands(1, level)
    plan = ndwt.Plan([N], ["db4"], torch_real(kind), cplx, pres_l2_norm=True, max_level=level, howmany=K)
    rng = np.random.default_rng(41)
    sig = np.stack([piecewise(N), 0.5 * piecewise(N)[::-1], np.zeros(N)])          # the last item: noise alone
    x = np.zeros((K, N * comp))
    for part in range(comp):
        x[:, part::comp] = (sig if part == 0 else 0.3 * sig) + sigma * rng.standard_normal((K, N))
    xt = torch.from_numpy(x.astype(rdt).reshape(-1)).cuda()
    yt = torch.zeros(nb * K * N * comp, dtype=torch_real(kind), device="cuda")
    plan.dec(xt.data_ptr(), yt.data_ptr(), level, stream())
    yh = yt.cpu().numpy()
    gains = ndwt.band_gains([N], "db4", level, 1)
    sigmas = np.array([sigma, sigma, 0.8 * sigma])

    def compare(got_t, got_r, block, s, n, rounds, what):
        stats = lambda row: reference(kind, block, row, True)
        want_t, want_r = search(kind, N, n, s, rounds, stats)
        scale = n * comp * s * s
        if abs(got_t - want_t) > 1e-12 * want_t:
            at = float(sure(comp, n, s, [got_t], stats([got_t]))[0])
            assert abs(at - want_r) <= 1e-9 * scale, (what, got_t, want_t, at, want_r)
        assert abs(got_r - want_r) <= 1e-9 * scale and got_r <= scale, (what, got_r, want_r)

    with ndwt.kernel_trace() as recs:
        thr, est = plan.sure_thresholds_items(yt.data_ptr(), level, sigmas, 3, stream())
    assert [r.family for r in recs].count("BandRisk") == 3           # the detail bands are read `rounds` times
    assert thr.shape == (K, nb) and est.shape == (K, nb) and not thr[:, 0].any() and not est[:, 0].any()
    thr1, est1 = plan.sure_thresholds_items(yt.data_ptr(), level, sigmas, 1, stream())
    for j in range(K):
        for b in range(1, nb):
            blk = yh[(b * K + j) * N * comp:(b * K + j + 1) * N * comp]
            s = sigmas[j] * gains[b]
            compare(thr[j, b], est[j, b], blk, s, float(N), 3, f"item {j} band {b}")
            compare(thr1[j, b], est1[j, b], blk, s, float(N), 1, f"item {j} band {b}, one round")
            assert 0.0 <= thr[j, b] <= s * np.sqrt(2 * np.log(N)) * (1 + 1e-6)
    assert (est <= est1).all()                                    # further rounds only improve on the first
    assert thr[:, 1:].any()
    # pooled: a band is all K items, n = K N elements, N still the elements of one item
    pthr, pest = plan.sure_thresholds(yt.data_ptr(), level, sigma, 0, stream())      # (0 rounds: the default, 3)
    assert pthr.shape == (nb,) and pthr[0] == 0 and pest[0] == 0
    for b in range(1, nb):
        compare(pthr[b], pest[b], yh[b * K * N * comp:(b + 1) * K * N * comp], sigma * gains[b], float(K * N), 3, f"pooled band {b}")
    # sigma = 0: nothing to search, nothing is read
    with ndwt.kernel_trace() as recs:
        zthr, zest = plan.sure_thresholds(yt.data_ptr(), level, 0.0, 3, stream())
    assert recs == [] and not zthr.any() and not zest.any()
    # the rows are what shrink and denoise take
    out = torch.zeros_like(xt)
    plan.denoise_bands_items(xt.data_ptr(), out.data_ptr(), level, thr, False, stream())
    assert torch.isfinite(out).all() and float((out - xt).abs().max()) > 0
    assert same(yt.cpu().numpy(), yh)


def test_the_classes_band_risk_and_sure_thresholds_with_the_hybrid_rule():
    K, n, level = 2, 1024, 3
    w = ndwt.nd_dwt_1D("db4", n, "pres_l2_norm", 1, "batch", K, "precision", "double")
    rng = np.random.default_rng(3)
    t = np.arange(n)
    busy = 4.0 * np.sin(2 * np.pi * t / 12.0)                    # its energy lies in the level-3 detail band (band 1), far above the noise
    x = np.stack([busy + 0.1 * rng.standard_normal(n), 0.25 * rng.standard_normal(n)], axis=1)   # item 1: zeros plus noise
    xt = torch.from_numpy(x).cuda()
    nb = ndwt.num_bands(1, level)
    y = w.dec(xt, level)
    yh = y.cpu().numpy()                                          # [n, K, bands]
    # band_risk: the dict, per item and pooled, against numpy
    cand = np.tile(np.array([0.0, 0.2, np.inf]), (K, nb, 1))
    r = w.band_risk(y, cand, per_item=True)
    assert set(r) == {"count", "energy", "invsum"} and all(v.shape == (K, nb, 3) for v in r.values())
    for j in range(K):
        for b in range(nb):
            a = np.abs(yh[:, j, b])
            assert r["count"][j, b].tolist() == [(a <= 0).sum(), (a <= 0.2).sum(), n]
            assert abs(r["energy"][j, b, 1] - (a[a <= 0.2] ** 2).sum()) <= n * 2.0 ** -52 * (a[a <= 0.2] ** 2).sum()
    rp = w.band_risk(y, cand[0])
    assert rp["count"].shape == (nb, 3) and np.array_equal(rp["count"], r["count"].sum(axis=0)) and not rp["invsum"].any()
    # sure_thresholds: the plan's search, then the hybrid rule written out here
    sig = w.estimate_sigma(xt, per_item=True)
    gains = w.band_gains(level)
    s = np.outer(sig, gains)
    plain = w.sure_thresholds(xt, level, per_item=True, hybrid=False)
    thr = w.sure_thresholds(xt, level, per_item=True)
    assert plain.shape == thr.shape == (K, nb) and not thr[:, 0].any() and not plain[:, 0].any()
    l2 = (yh ** 2).sum(axis=0)                                    # [K, bands]
    sparse = (l2 / (s * s) - n) / n <= np.log2(n) ** 1.5 / np.sqrt(n)
    assert sparse[1, 1:].all() and not sparse[0, 1]              # the noise-only item is too sparse for the estimate, band 1 of the other is not
    want = np.where(sparse, s * np.sqrt(2 * np.log(n)), plain)
    want[:, 0] = 0.0
    assert np.allclose(thr, want, rtol=1e-14, atol=0)
    assert (plain[1, 1:] <= want[1, 1:] * (1 + 1e-12)).all()     # the search never leaves [0, the universal threshold]
    pooled = w.sure_thresholds(xt, level, rounds=2)
    assert pooled.shape == (nb,) and pooled[0] == 0 and (pooled[1:] >= 0).all() and pooled.any()
    out = w.denoise(xt, level, thr)
    assert out.shape == xt.shape and torch.isfinite(out).all()


def test_every_refusal_names_its_argument_and_launches_nothing():
    plan = ndwt.Plan([96], ["db2"], torch.float32, False, max_level=3, howmany=5)
    items, N, level, nb = 5, 96, 2, 3
    c = Coefs("f32", items, N, nb, 0, 5)
    lib = ndwt.lib()
    err = lambda: lib.ndwt_last_error().decode()
    DP = ctypes.POINTER(ctypes.c_double)
    v = (ctypes.c_double * 512)(*[-1.0] * 512)
    t = (ctypes.c_double * 64)(*[-3.0] * 64)

    def table(fill=0.5, **at):
        a = np.full((items, nb, 8), fill)
        for k, val in at.items():
            a[tuple(int(d) for d in k.split("_")[1:])] = val
        return np.ascontiguousarray(a)
    good = table()
    gp = good.ctypes.data_as(DP)
    with ndwt.kernel_trace() as recs:
        for f, per in ((lib.ndwt_band_risk, False), (lib.ndwt_band_risk_items, True)):
            for args, word in (((None, 0, level, 8, gp, v), "y_dev"), ((c.ptr, 0, level, 8, None, v), "cand"), ((c.ptr, 0, level, 8, gp, None), "(risk)"),
                               ((c.ptr, 0, 0, 8, gp, v), "level 0"), ((c.ptr, 0, 4, 8, gp, v), "level 4"), ((c.ptr, items * N - 1, level, 8, gp, v), "pitch"),
                               ((c.ptr, 0, level, 0, gp, v), "nc = 0"), ((c.ptr, 0, level, 9, gp, v), "nc = 9")):
                assert f(plan._h, *args, None) == 1 and word in err(), (word, err())
            for bad, word in ((table(at_0_2_3=np.nan), "band 2, position 3"), (table(at_0_1_1=-0.5), "band 1, position 1"),
                              (table(at_0_0_0=np.nan), "band 0, position 0")):
                assert f(plan._h, c.ptr, 0, level, 8, bad.ctypes.data_as(DP), v, None) == 1 and word in err(), (word, err())
                assert ("item 0" in err()) == per
        bad = table(at_4_2_7=-1.0)
        assert lib.ndwt_band_risk_items(plan._h, c.ptr, 0, level, 8, bad.ctypes.data_as(DP), v, None) == 1 and "item 4, band 2, position 7" in err()
        sg = (ctypes.c_double * 5)(*[0.3] * 5)
        for args, word in (((None, 0, level, 0.3, 3, t, v), "y_dev"), ((c.ptr, 0, level, 0.3, 3, None, v), "thresholds"), ((c.ptr, 0, 4, 0.3, 3, t, v), "level 4"),
                           ((c.ptr, 0, level, -0.1, 3, t, v), "sigma"), ((c.ptr, 0, level, float("nan"), 3, t, v), "sigma"),
                           ((c.ptr, 0, level, float("inf"), 3, t, v), "sigma"), ((c.ptr, 0, level, 0.3, -1, t, v), "rounds = -1"),
                           ((c.ptr, 0, level, 0.3, 9, t, v), "rounds = 9"), ((c.ptr, items * N - 1, level, 0.3, 3, t, v), "pitch")):
            assert lib.ndwt_sure_thresholds(plan._h, *args, None) == 1 and word in err(), (word, err())
        assert lib.ndwt_sure_thresholds_items(plan._h, c.ptr, 0, level, None, 3, t, v, None) == 1 and "sigma" in err()
        sg[3] = -1.0
        assert lib.ndwt_sure_thresholds_items(plan._h, c.ptr, 0, level, sg, 3, t, v, None) == 1 and "sigma of item 3" in err()
    assert recs == [] and list(v) == [-1.0] * 512 and list(t) == [-3.0] * 64 and c.unchanged()
    with pytest.raises(ndwt.NdwtError, match="level 4"):
        plan.band_risk(c.ptr, 4, np.full((ndwt.num_bands(1, 4), 8), 0.5), stream())
    with pytest.raises(ValueError, match="candidates per block"):
        plan.band_risk(c.ptr, level, np.zeros((nb, 9)), stream())
    with pytest.raises(ValueError, match="array of candidate thresholds expected"):
        plan.band_risk_items(c.ptr, level, np.zeros((nb, 8)), stream())
