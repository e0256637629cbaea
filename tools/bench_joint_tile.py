#!/usr/bin/env python3
"""The two forms of the joint shrinkage (ndwt_shrink_joint) and of the group norms (ndwt_group_norms_dev) on batches of signals, hipEvent
timing: the chunk form JointShrink / GroupNorms (variant_inv 9) against the tile form JointTile / GroupNormsTile (variant_inv 11), next to
torch and to the bytes at the measured rates.  The table joint_route's default (csrc/ndwt_select.h) is read from.

Per cell (items x item length, a batched 1-D plan, random coefficients -- the calls need no transform -- thresholds at about the median
group magnitude) one line for the shrink and one for the norms:

  shrink   chunk form, tile form, tile / chunk, torch (pow / sum / sqrt / clamp / mul per band, as tools/bench_joint.py), two reads + one
           write at --read-gbs and --copy-gbs ("read linear" and "copy 1->1 linear" of tools/micro/stream_pattern of the same session)
  norms    chunk form, tile form, tile / chunk, torch, one read at --read-gbs

The array is restored from a copy before every timed shrink, outside the events.  Median of 20 timed calls in 4 interleaved rounds of 5
after 5 warm-ups of each line, as tools/bench_joint.py.  Before timing, the tile form's array and its nnz / max must equal the chunk
form's bit for bit, and the trace must name the form asked for.  Cells whose array would exceed --max-mib are left out.

    python tools/bench_joint_tile.py [--kinds f32,f64] [--levels 1,4] [--items 16,64,...] [--lengths 1024,...] [--extra stack2:512x32,stack3:256x8]
                                     [--max-mib 256] [--copy-gbs N] [--read-gbs N] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--kinds", default="f32,f64")
ap.add_argument("--levels", default="1,4")
ap.add_argument("--items", default="16,64,256,1024,4096")
ap.add_argument("--lengths", default="1024,4096,16384,65536")
ap.add_argument("--extra", default="stack2:512x32,stack3:256x8", help="the stacks of tools/bench_joint.py's table, level 1 (not bound by --max-mib)")
ap.add_argument("--max-mib", type=float, default=256.0)
ap.add_argument("--copy-gbs", type=float, default=0.0)
ap.add_argument("--read-gbs", type=float, default=0.0)
ap.add_argument("--out", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ndwt_amd as ndwt  # noqa: E402

s = torch.cuda.current_stream().cuda_stream
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def timed_interleaved(fns, before=None, rounds=4, per=5, warm=5):
    for k, f in fns.items():
        for _ in range(warm):
            if before and k in before:
                before[k]()
            f()
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            for _ in range(per):
                if before and k in before:
                    before[k]()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                ts[k].append(e0.elapsed_time(e1) * 1e3)
    return {k: statistics.median(v) for k, v in ts.items()}


def torch_shrink(bands, K, thr):
    for v, t in zip(bands, thr):
        v = v.view(K, -1)
        m = v.pow(2).sum(0).sqrt()
        g = (1 - t / m).clamp(min=0)
        v.mul_(g)


def torch_norms(bands, K):
    rows = []
    for v in bands:
        sq = v.view(K, -1).pow(2).sum(0, dtype=torch.float64)
        m = sq.sqrt()
        rows.append(torch.stack([m.sum(), sq.sum(), m.max(), torch.count_nonzero(sq).double()]))
    return torch.stack(rows)


def cell(name, make_plan, K, n, nb, level, rdt):
    N = K * n
    plans = {v: make_plan().set_variant(-1, v) for v in (9, 11)}
    gen = torch.Generator(device="cuda").manual_seed(7)
    y0 = torch.randn(nb * N, dtype=rdt, device="cuda", generator=gen)
    y = y0.clone()
    bands = [y[b * N:(b + 1) * N] for b in range(nb)]
    thr = np.full(nb, float(np.sqrt(K - 0.5)))                  # about the median of a chi variable of K degrees
    restore = lambda: y.copy_(y0)                               # noqa: E731
    out = torch.empty(nb * 4, dtype=torch.float64, device="cuda")
    shrink = {v: (lambda p=p: p.shrink_joint(y.data_ptr(), level, thr, False, s)) for v, p in plans.items()}
    norms = {v: (lambda p=p: p.group_norms_dev(y.data_ptr(), level, out.data_ptr(), s)) for v, p in plans.items()}
    # the values first: the two forms bit for bit, and the form asked for is the one that ran
    got, nrm = {}, {}
    for v in (9, 11):
        restore()
        with ndwt.kernel_trace() as recs:
            norms[v]()
            nrm[v] = out.clone()
            shrink[v]()
        fams = [r.family for r in recs]
        assert fams[0] == ("GroupNormsTile" if v == 11 else "GroupNorms") and fams[-1] == ("JointTile" if v == 11 else "JointShrink"), (name, v, fams)
        got[v] = y.clone()
        grids = (recs[0].grid[0], recs[-1].grid[0])
    assert torch.equal(got[9].view(torch.uint8), got[11].view(torch.uint8)), name
    a, b = nrm[9].view(nb, 4), nrm[11].view(nb, 4)
    assert torch.equal(a[:, 2:], b[:, 2:]) and torch.allclose(a[:, :2], b[:, :2], rtol=1e-12), name
    survive = float((got[11] != 0).double().mean())
    assert 0.2 < survive < 0.8, (name, survive)
    del got
    restore()
    t = timed_interleaved({"s9": shrink[9], "s11": shrink[11], "st": lambda: torch_shrink(bands, K, thr),
                           "n9": norms[9], "n11": norms[11], "nt": lambda: torch_norms(bands, K)}, before={"s9": restore, "s11": restore, "st": restore})
    gb = nb * N * y.element_size() / 1e9
    f21 = gb / args.read_gbs * 1e6 + 2 * gb / args.copy_gbs * 1e6 if args.copy_gbs > 0 and args.read_gbs > 0 else 0.0
    f1 = gb / args.read_gbs * 1e6 if args.read_gbs > 0 else 0.0
    say(f"{name:34s} {nb} bands {gb * 1e3:7.1f} MB  tile grid {grids[1]:7d} | shrink us: chunk {t['s9']:9.1f}  tile {t['s11']:9.1f}  tile/chunk {t['s11'] / t['s9']:5.2f}  "
        f"torch {t['st']:9.1f}  2R+1W {f21:7.1f} | norms us: chunk {t['n9']:9.1f}  tile {t['n11']:9.1f}  tile/chunk {t['n11'] / t['n9']:5.2f}  torch {t['nt']:9.1f}  1R {f1:7.1f}")
    say(json.dumps({"cell": name, "items": K, "item_scalars": n, "bands": nb, "level": level, "us": {k: round(v, 1) for k, v in t.items()},
                    "floor_2r1w_us": round(f21, 1), "floor_1r_us": round(f1, 1)}))
    del plans, y, y0, bands
    torch.cuda.empty_cache()


say(f"# python tools/bench_joint_tile.py --copy-gbs {args.copy_gbs:.0f} --read-gbs {args.read_gbs:.0f}   (us per call, medians of 20)")
for kind in args.kinds.split(","):
    rdt = torch.float32 if kind == "f32" else torch.float64
    esize = 4 if kind == "f32" else 8
    for level in (int(v) for v in args.levels.split(",")):
        nb = ndwt.num_bands(1, level)
        for n in (int(v) for v in args.lengths.split(",")):
            for K in (int(v) for v in args.items.split(",")):
                if nb * K * n * esize > args.max_mib * 2 ** 20:
                    continue
                cell(f"batch:{kind}:{K}x{n}:L{level}", lambda: ndwt.Plan([n], ["db4"], rdt, False, True, "reference", max_level=level, howmany=K), K, n, nb, level, rdt)
    for extra in [e for e in args.extra.split(",") if e]:
        what, dims = extra.split(":")
        a, K = (int(v) for v in dims.split("x"))
        if what == "stack3":
            cell(f"{what}:{kind}:{dims}:L1", lambda: ndwt.Plan([a, a, a, K], ["db4"] * 3 + [None], rdt, False, True, "reference", max_level=1, axes=(0, 1, 2)), K, a ** 3, 8, 1, rdt)
        else:
            cell(f"{what}:{kind}:{dims}:L1", lambda: ndwt.Plan([a, a, K], ["db4", "db4", None], rdt, False, True, "reference", max_level=1, axes=(0, 1)), K, a * a, 4, 1, rdt)

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
