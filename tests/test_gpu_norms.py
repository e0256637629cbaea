"""The band norms on the device: ndwt_band_norms, ndwt_band_norms_items, ndwt_band_norms_dev and the classes' band_norms, l1_norm,
sparsity and bayes_thresholds.

The sums need no transform: the coefficient array is ARBITRARY DATA written by the test (tests/norms_cases.py: the items of
tests/items_cases.py -- an all-equal item, an item with a NaN --, an all-zero item with one -0, integer-valued items), the plan only
supplies the sizes, the items and the data kind.  Every array lies between guard words, the bands on a pitch have guard words between
them, and the whole buffer is compared with its copy afterwards.  The shapes are the smallest at which each form of the kernel can go
wrong:

  1-D, n = 37, db2, float, level 2                      element-wise, below one workgroup
  batch 5 x 96, db2, complex64, level 3                 the 4-scalar form, 4 bands x 5 items
  batch 2 x 20000, db4, float and double, level 1       chunks > 1 with a ragged last chunk, so NormsFinish runs; once more with
                                                        set_tuning(target_blocks=1): one chunk and one launch
  stack 8 x 12 x 3 items, db2, complex128, level 2      7 bands, band_pitch = ndwt_band_pitch, guard words between and behind the bands
  3-D 8 x 8 x 8, db2, double, level 2                   15 bands; the array one element off a 32-byte boundary: the element-wise form
  interleaved, inner = 3, 16 x 16, db1, float, level 1  the items of ndwt_plan_create_interleaved (two blocks of 768 scalars); and
                                                        15 x 15: items of 675 scalars, a length that is no multiple of 4
  1-D n = 37 complex64, 3-D 8 x 8 x 8 complex128        complex data in the element-wise form

  values     against numpy on the host copy, with the tolerances and the exact cases of tests/norms_cases.py (derived there)
  select     the max of every block equals band_select_items(k = elements - 1) bit for bit
  pooled     the pooled call against the per-item rows: nnz (their sum) and max exactly, l1 and l2sq within n 2^-52
  device     band_norms_dev equals the host form bit for bit; two calls return the same bits; the input is untouched
  trace      chunks = 1: exactly one BandNorms record; chunks > 1: one BandNorms and one NormsFinish, with the grids norms_chunks gives
  shrink     after shrink_bands(hard) nnz[b] is numpy's count of |c| > thr[b]; a threshold of 0 leaves the statistics of its band unchanged
  classes    band_norms, l1_norm and sparsity against the same numpy sums; bayes_thresholds against its formula in numpy, per item, with
             one signal of noise alone (the v_b = 0 branch), and denoise accepts the result
  refusals   name the argument and launch nothing
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import ndwt_amd as ndwt
from items_cases import build_named_shim
from norms_cases import L1, L2SQ, MAX, NNZ, check_array, check_block, norms_array
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
    if shape == "inner-3-16x16":
        return ndwt.Plan([16, 16], ["db1", "db1"], rdt, cplx, max_level=1, inner=3, howmany=2), 2, 768, 2, 1, False, 0, True
    if shape == "inner-3-15x15":
        return ndwt.Plan([15, 15], ["db1", "db1"], rdt, cplx, max_level=1, inner=3, howmany=2), 2, 675, 2, 1, False, 0, False
    raise ValueError(shape)


CASES = [("f32", "1d-37"), ("c64", "batch-5x96"), ("f32", "batch-2x20000"), ("f64", "batch-2x20000"), ("c128", "stack-3x8x12"),
         ("f64", "3d-8x8x8-skew"), ("f32", "inner-3-16x16"), ("f32", "inner-3-15x15"),
         # complex data in the element-wise form too: its float magnitude is rounded differently from the 4-scalar form's (norms_magnitude)
         ("c64", "1d-37"), ("c128", "3d-8x8x8-skew")]


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
def test_the_norms_of_every_block(shim, kind, shape):
    rdt, cplx = KINDS[kind]
    plan, items, N, axes, level, pitched, skew, vec = make_case(kind, shape)
    comp = 2 if cplx else 1
    assert plan.items == items
    nb = ndwt.num_bands(axes, level)
    pitch = plan.band_pitch() if pitched else 0
    assert not pitched or pitch >= items * N
    c = Coefs(kind, items, N, nb, pitch, zlib.crc32(f"{kind}-{shape}".encode()) % 100000, skew)
    assert vec == (c.ptr % (4 * c.host.itemsize) == 0 and c.bs % 4 == 0 and (N * comp) % 4 == 0)
    n = N * comp
    fam = {"T": tname(kind), "COMP": comp}

    def traced(f, n_scalars, n_items, target=0):
        """f() with its trace checked: one BandNorms on bands x items x chunks workgroups, and one NormsFinish where chunks > 1"""
        v = c.ptr % (4 * c.host.itemsize) == 0 and c.bs % 4 == 0 and n_scalars % 4 == 0
        chunks = int(shim.sel_norms_chunks(n_scalars, comp, int(v), nb, n_items, cus(), target))
        with ndwt.kernel_trace() as recs:
            out = f()
        assert len(recs) == (1 if chunks == 1 else 2), recs
        assert recs[0].family == "BandNorms" and recs[0].params == dict(fam, VEC=v), recs[0]
        assert recs[0].grid == (nb * n_items * chunks, 1, 1) and recs[0].block == (256, 1, 1), (recs[0], chunks)
        if chunks > 1:
            assert recs[1].family == "NormsFinish" and recs[1].grid == (nb * n_items, 1, 1) and recs[1].block == (64, 1, 1), recs[1]
        return out, chunks

    per, chunks = traced(lambda: plan.band_norms_items(c.ptr, level, stream(), band_pitch=pitch), n, items)
    assert per.shape == (items, nb, 4)
    if shape == "batch-2x20000":
        assert chunks == 2                                        # 5000 steps: two chunks of 9.77 turns, the last one ragged
    else:
        assert chunks == 1
    check_array(kind, c.flat, c.bs, items, N, nb, per, c.integer, f"{kind}-{shape}")
    pooled, pchunks = traced(lambda: plan.band_norms(c.ptr, level, stream(), band_pitch=pitch), items * n, 1)
    assert pooled.shape == (nb, 4) and (shape != "batch-2x20000" or pchunks == 4)
    for b in range(nb):
        check_block(kind, c.flat[b * c.bs:b * c.bs + items * n], pooled[b], f"{kind}-{shape} pooled band {b}", all((b, j) in c.integer for j in range(items)))
    # pooled against per item: nnz and max exactly, l1 and l2sq within n 2^-52 (n: the scalars of the pooled block)
    assert np.array_equal(pooled[:, NNZ], per[:, :, NNZ].sum(axis=0))
    with np.errstate(invalid="ignore"):
        assert np.array_equal(pooled[:, MAX], per[:, :, MAX].max(axis=0), equal_nan=True)   # (np.max keeps a NaN, as the kernel does)
        for s in (L1, L2SQ):
            want = per[:, :, s].sum(axis=0)
            ok = np.abs(pooled[:, s] - want) <= items * n * 2.0 ** -52 * np.abs(want)
            assert (ok | (np.isnan(want) & np.isnan(pooled[:, s]))).all(), (s, pooled[:, s], want)
    if items == 1:                                                # one item: the per-item call equals the pooled one
        assert same(per[0], pooled)
    # the max of every block is the select's last order statistic, bit for bit
    for b in range(nb):
        top = plan.band_select_items(c.ptr, level, b, [N - 1], stream(), band_pitch=pitch)
        assert np.array_equal(top[:, 0], per[:, b, MAX], equal_nan=True), (b, top[:, 0], per[:, b, MAX])
    # repeatability, and the device form
    assert same(plan.band_norms_items(c.ptr, level, stream(), band_pitch=pitch), per)
    assert same(plan.band_norms(c.ptr, level, stream(), band_pitch=pitch), pooled)
    raw = torch.full((1 + items * nb * 4 + 1,), -3.0, dtype=torch.float64, device="cuda")
    for per_item, want in ((True, per), (False, pooled)):
        raw.fill_(-3.0)
        _, ch = traced(lambda: plan.band_norms_dev(c.ptr, level, raw.data_ptr() + 8, per_item, stream(), band_pitch=pitch), n if per_item else items * n,
                       items if per_item else 1)
        got = raw.cpu().numpy()
        assert same(got[1:1 + want.size], want.reshape(-1)) and (got[1 + want.size:] == -3.0).all() and got[0] == -3.0
    if shape == "batch-2x20000":
        # one chunk and one launch on request: the same exact values, the sums within their bound (another order)
        plan.set_tuning(target_blocks=1)
        one, ch = traced(lambda: plan.band_norms_items(c.ptr, level, stream(), band_pitch=pitch), n, items, 1)
        assert ch == 1
        check_array(kind, c.flat, c.bs, items, N, nb, one, c.integer, f"{kind}-{shape} one chunk")
        assert same(one[..., NNZ], per[..., NNZ]) and same(one[..., MAX], per[..., MAX])
        plan.set_tuning(target_blocks=0)
        assert same(plan.band_norms_items(c.ptr, level, stream(), band_pitch=pitch), per)
    assert c.unchanged()                                          # the array, the guard words between and around the bands


def test_after_a_hard_shrink_nnz_counts_what_survives_and_a_zero_threshold_changes_nothing():
    plan = ndwt.Plan([96], ["db2"], torch.float32, False, max_level=3, howmany=5)
    items, N, level, nb = 5, 96, 3, 4
    rng = np.random.default_rng(17)
    host = rng.standard_normal(nb * items * N).astype(np.float32)
    y = torch.from_numpy(host).cuda()
    before = plan.band_norms(y.data_ptr(), level, stream())
    before_items = plan.band_norms_items(y.data_ptr(), level, stream())
    thr = np.array([0.0, 0.5, 0.0, 1.25])
    plan.shrink_bands(y.data_ptr(), level, thr, True, stream())
    after = plan.band_norms(y.data_ptr(), level, stream())
    after_items = plan.band_norms_items(y.data_ptr(), level, stream())
    bands = host.reshape(nb, items * N)
    for b in range(nb):
        if thr[b] == 0.0:
            assert same(after[b], before[b]) and same(after_items[:, b], before_items[:, b])
        else:
            assert after[b, NNZ] == np.count_nonzero(np.abs(bands[b]) > np.float32(thr[b]))
            assert np.array_equal(after_items[:, b, NNZ], (np.abs(bands[b].reshape(items, N)) > np.float32(thr[b])).sum(axis=1))
            assert after[b, MAX] == before[b, MAX] and after[b, L1] < before[b, L1]   # hard: what survives is unchanged


def test_the_classes_l1_norm_sparsity_and_band_norms():
    K, n, level = 5, 96, 3
    for prec, cplx in (("single", False), ("double", True)):
        w = ndwt.nd_dwt_1D("db2", n, "batch", K, "precision", prec)
        rng = np.random.default_rng(23)
        x = rng.standard_normal((n, K)) + (1j * rng.standard_normal((n, K)) if cplx else 0)
        xt = torch.from_numpy(x.astype({("single", False): np.float32, ("double", True): np.complex128}[(prec, cplx)])).cuda()
        y = w.shrink(w.dec(xt, level), 0.8, "hard")                # some exact zeros
        yh = y.cpu().numpy().astype(np.complex128 if cplx else np.float64)   # [n, K, bands]
        nb = yh.shape[-1]
        a = np.abs(yh)
        for per_item in (False, True):
            ax = (0,) if per_item else (0, 1)
            # n 2^-52 for the scalars of a block; complex double: numpy's |c| is hypot, the kernel's sqrt(re^2 + im^2) -- 4 u apart at most
            tol = n * (1 if per_item else K) * (2 if cplx else 1) * 2.0 ** -52 + (4 * 2.0 ** -53 if cplx else 0)
            v = w.band_norms(y, per_item=per_item)
            assert set(v) == {"l1", "l2sq", "max", "nnz"} and all(v[k].shape == ((K, nb) if per_item else (nb,)) for k in v)
            assert np.allclose(v["l1"], a.sum(axis=ax), rtol=tol, atol=0) and np.allclose(v["l2sq"], (yh.real ** 2 + yh.imag ** 2).sum(axis=ax), rtol=tol, atol=0)
            assert np.array_equal(v["nnz"], (yh != 0).sum(axis=ax))
            assert np.allclose(v["max"], a.max(axis=ax), rtol=4 * 2.0 ** -53 if cplx else 0, atol=0)
            wts = np.arange(1.0, nb + 1)
            assert np.allclose(w.l1_norm(y, per_item=per_item), a.sum(axis=ax)[..., 1:].sum(axis=-1), rtol=2 * tol, atol=0)
            assert np.allclose(w.l1_norm(y, wts, per_item=per_item), a.sum(axis=ax) @ wts, rtol=2 * tol, atol=0)
            sp = w.sparsity(y, per_item=per_item)
            assert np.array_equal(sp, (yh != 0).sum(axis=ax).sum(axis=-1) / (yh.size / (K if per_item else 1)))
            assert (np.shape(sp) == (K,)) if per_item else isinstance(sp, float)
        assert 0.0 < w.sparsity(y) < 1.0 and isinstance(w.l1_norm(y), float)


def test_bayes_thresholds_is_its_formula_per_item_and_denoise_takes_it():
    """a batch of 3 noisy step signals with different noise levels; the last one is noise alone, and uniform noise: the median-based sigma
    overestimates the standard deviation of such flat-topped noise (by 7 % and more in every band at this size: tests on the oracle), so
    its bands take the v_b = 0 branch and their thresholds are the blocks' maxima"""
    K, n, level = 3, 1024, 2
    w = ndwt.nd_dwt_1D("db2", n, "pres_l2_norm", 1, "batch", K, "precision", "double")
    rng = np.random.default_rng(0)
    step = np.where(np.arange(n) < n // 2, 1.0, -0.5) + np.where(np.arange(n) % 256 < 128, 0.75, 0.0)
    x = np.stack([step + 0.05 * rng.standard_normal(n), 2 * step + 0.2 * rng.standard_normal(n), 0.3 * np.sqrt(3) * rng.uniform(-1, 1, n)], axis=1)
    xt = torch.from_numpy(x).cuda()
    thr = w.bayes_thresholds(xt, level, per_item=True)
    nb = ndwt.num_bands(1, level)
    assert thr.shape == (K, nb) and (thr[:, 0] == 0).all() and (thr[:, 1:] > 0).all()
    # the formula in numpy, from the coefficients on the host and estimate_sigma
    yh = w.dec(xt, level).cpu().numpy()                           # [n, K, bands]
    s = np.outer(w.estimate_sigma(xt, per_item=True), w.band_gains(level))
    l2 = np.stack([[(yh[:, j, b] ** 2).sum() for b in range(nb)] for j in range(K)])
    var = np.maximum(l2 / n - s * s, 0.0)
    assert (var[:2, 1:] > 0).all() and (var[2, 1:] == 0).all()     # the signals carry signal; the noise-only row does not
    want = np.where(var > 0, s * s / np.sqrt(np.where(var > 0, var, 1.0)), np.abs(yh).max(axis=0))
    want[:, 0] = 0.0
    assert np.array_equal(thr[2, 1:], np.abs(yh[:, 2, 1:]).max(axis=0))          # the maxima, exactly: the band goes to zero
    # l2sq is within n 2^-52 of numpy's; var = l2sq / n - s^2 loses relative accuracy by l2sq / (n var), the threshold half of that
    amp = (l2 / n) / np.where(var > 0, var, 1.0)
    assert (np.abs(thr - want) <= (n * 2.0 ** -52 * amp + 4 * 2.0 ** -53) * np.abs(want)).all(), (thr, want)
    pooled = w.bayes_thresholds(xt, level)
    assert pooled.shape == (nb,) and pooled[0] == 0 and (pooled[1:] > 0).all()
    # denoise accepts the table: it is rec(shrink(dec(x), thr)); the noise-only signal keeps its approximation alone (no detail coefficient
    # lies above its band's maximum)
    out = w.denoise(xt, level, thr)
    assert out.shape == xt.shape and torch.isfinite(out).all()
    ys = w.shrink(w.dec(xt, level), thr)
    assert not ys.cpu().numpy()[:, 2, 1:].any() and ys.cpu().numpy()[:, :2, 1:].any()
    assert float((out - w.rec(ys)).abs().max()) <= 1e-12 * float(xt.abs().max())


def test_every_refusal_names_its_argument_and_launches_nothing():
    plan = ndwt.Plan([96], ["db2"], torch.float32, False, max_level=3, howmany=5)
    items, N, level, nb = 5, 96, 2, 3
    c = Coefs("f32", items, N, nb, 0, 5)
    lib = ndwt.lib()
    err = lambda: lib.ndwt_last_error().decode()
    v = (ctypes.c_double * 64)(*[-1.0] * 64)
    out = torch.full((64,), -2.0, dtype=torch.float64, device="cuda")
    with ndwt.kernel_trace() as recs:
        for f in (lib.ndwt_band_norms, lib.ndwt_band_norms_items):
            for args, word in (((None, 0, level, v), "y_dev"), ((c.ptr, 0, level, None), "(norms)"), ((c.ptr, 0, 0, v), "level 0"), ((c.ptr, 0, 4, v), "level 4"),
                               ((c.ptr, items * N - 1, level, v), "pitch")):
                assert f(plan._h, *args, None) == 1 and word in err(), (word, err())
        for per_item in (0, 1):
            for args, word in (((None, 0, level, per_item, out.data_ptr()), "y_dev"), ((c.ptr, 0, level, per_item, None), "norms_dev"),
                               ((c.ptr, 0, level, per_item, out.data_ptr() + 4), "norms_dev must be 8-byte aligned"), ((c.ptr, 0, 4, per_item, out.data_ptr()), "level 4"),
                               ((c.ptr, items * N - 1, level, per_item, out.data_ptr()), "pitch")):
                assert lib.ndwt_band_norms_dev(plan._h, *args, None) == 1 and word in err(), (word, err())
    assert recs == [] and list(v) == [-1.0] * 64 and (out == -2.0).all().item() and c.unchanged()
    with pytest.raises(ndwt.NdwtError, match="level 4"):
        plan.band_norms(c.ptr, 4, stream())
