#!/usr/bin/env python3
"""Plans over interleaved samples with ONE filtered axis (ndwt_plan_create_interleaved, ndim = 1) against what a caller did before them,
3 levels, device-resident data, hipEvent timing:

  (a) the batched 1-D plan of the PARENT build (--parent-lib: its libndwt_hip.so, loaded into this process beside this build's; without
      it this build's): permute the filtered axis to the front (.contiguous()), run the plan, permute every band back -- the rec the
      other way round;
  (b) the new plan, one launch per level (variants 9 / 9);
  (c) the new plan with the cascaded march forced (FwdMC / InvMC, variants 11 / 11).

Interleaved batches: after 5 warm-ups of every line, 4 rounds of 5 timed calls per line, the lines taking turns; the median of a line's 20.
The unbatched controls (--controls): plans this build did not mean to change, on this build against the parent, the same way (10 rounds
of 10): a batched 1-D plan `many:KxN` and an unbatched array `kind:n4xn3xn2xn1`.

    python tools/bench_interleaved.py [--parent-lib PATH] [--shapes f32:1x32x65536,...] [--wnames db2,db4] [--level 3] [--out FILE]

A shape is kind:K x n x inner -- K items, the filtered axis of n samples, `inner` elements per sample (slowest first).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--shapes", default="f32:1x32x65536,c64:1x32x65536,f32:1x64x262144,f32:1x64x1048576,f64:1x32x65536,f32:64x4096x64")
ap.add_argument("--wnames", default="db2,db4")
ap.add_argument("--level", type=int, default=3)
ap.add_argument("--controls", default="many:4096x4096,f32:16x64x64x64")
ap.add_argument("--out", default=None, help="also append every printed line to this file (profiles/bench_interleaved.txt)")
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import ndwt_amd as ndwt  # noqa: E402

KINDS = {"f32": (torch.float32, False), "c64": (torch.float32, True), "f64": (torch.float64, False), "c128": (torch.float64, True)}
level = args.level
s = torch.cuda.current_stream().cuda_stream
_out = open(args.out, "a") if args.out else None


def say(line):
    print(line, flush=True)
    if _out:
        _out.write(line + "\n")
        _out.flush()


class RawPlan:
    """a plan through the C ABI of any build of the library (the parent's knows nothing newer): howmany = None -> ndwt_plan_create,
    a number -> the batched 1-D plan of ndwt_plan_create_many"""

    def __init__(self, lib, dims, rdt, cplx, wname, howmany=None):
        self.lib, self.h = lib, ctypes.c_void_p(None)
        d = len(dims)
        head = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]
        lib.ndwt_plan_create.argtypes = head + [ctypes.POINTER(ctypes.c_char_p)] + [ctypes.c_int] * 6
        lib.ndwt_plan_create_many.argtypes = head + [ctypes.c_int64, ctypes.POINTER(ctypes.c_char_p)] + [ctypes.c_int] * 6
        for f in (lib.ndwt_dec, lib.ndwt_rec):
            f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        lib.ndwt_plan_destroy.argtypes = [ctypes.c_void_p]
        tail = (0 if rdt == torch.float32 else 1, int(cplx), 1, 0, level, torch.cuda.current_device())
        dims_c, names_c = (ctypes.c_int64 * d)(*dims), (ctypes.c_char_p * d)(*[wname.encode()] * d)
        if howmany is None:
            rc = lib.ndwt_plan_create(ctypes.byref(self.h), d, dims_c, names_c, *tail)
        else:
            rc = lib.ndwt_plan_create_many(ctypes.byref(self.h), d, dims_c, howmany, names_c, *tail)
        assert rc == 0, rc

    def dec(self, x, y):
        assert self.lib.ndwt_dec(self.h, x, y, level, s) == 0

    def rec(self, y, x):
        assert self.lib.ndwt_rec(self.h, y, x, level, s) == 0

    def close(self):
        self.lib.ndwt_plan_destroy(self.h)


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def interleaved(fns, rounds=4, per_round=5, warm=5):
    """{name: fn} -> {name: (median us, min, max)}"""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ts[k] += [once(fn) for _ in range(per_round)]
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


this_lib = ndwt.lib()
parent_lib = ctypes.CDLL(os.path.abspath(args.parent_lib)) if args.parent_lib else None
say(f"device: {torch.cuda.get_device_name()}; parent build: {'loaded from ' + os.path.basename(args.parent_lib) if parent_lib else 'none (line (a) runs this build)'}")

for shape in [v for v in args.shapes.split(",") if v]:
    kind, dd = shape.split(":")
    K, n, inner = (int(v) for v in dd.split("x"))
    rdt, cplx = KINDS[kind]
    tdt = (torch.complex64 if rdt == torch.float32 else torch.complex128) if cplx else rdt
    esize = (4 if rdt == torch.float32 else 8) * (2 if cplx else 1)
    nb, vol = 1 + level, K * n * inner
    for wname in args.wnames.split(","):
        x = torch.randn(vol, dtype=tdt, device="cuda")
        y = torch.randn(nb * vol, dtype=tdt, device="cuda")
        out_y, out_x = torch.empty_like(y), torch.empty_like(x)
        # (a): the filtered axis to the front, the batched 1-D plan over K * inner signals, every band back
        pa = RawPlan(parent_lib or this_lib, [n], rdt, cplx, wname, howmany=K * inner)

        def dec_permuted():
            xt = x.view(K, n, inner).permute(0, 2, 1).contiguous()
            yt = torch.empty((nb, K, inner, n), dtype=tdt, device="cuda")
            pa.dec(xt.data_ptr(), yt.data_ptr())
            out_y.view(nb, K, n, inner).copy_(yt.permute(0, 1, 3, 2))

        def rec_permuted():
            yt = y.view(nb, K, n, inner).permute(0, 1, 3, 2).contiguous()
            xt = torch.empty((K, inner, n), dtype=tdt, device="cuda")
            pa.rec(yt.data_ptr(), xt.data_ptr())
            out_x.view(K, n, inner).copy_(xt.permute(0, 2, 1))
        name_a = "(a) permute, batched 1-D plan" + (" of the parent" if parent_lib else "") + ", permute back"
        dec, rec, plans = {name_a: dec_permuted}, {name_a: rec_permuted}, []
        for name, v in (("(b) interleaved plan, 9 / 9", 9), ("(c) interleaved plan, cascade forced (11 / 11)", 11)):
            p = ndwt.Plan([n], [wname], rdt, cplx, True, "reference", max_level=level, inner=inner, howmany=K)
            p.set_variant(fwd=v, inv=v)
            plans.append(p)
            dec[name] = (lambda p=p: p.dec(x.data_ptr(), out_y.data_ptr(), level, s))
            rec[name] = (lambda p=p: p.rec(y.data_ptr(), out_x.data_ptr(), level, s))
            with ndwt.kernel_trace() as recs:
                dec[name]()
                rec[name]()
            say(f"    {name}: {p.describe()}; launches: {', '.join(f'{r.family}' + (str(r.params['NLEV']) if 'NLEV' in r.params else '') + f' x{r.grid[0]}' for r in recs)}")
        td, tr = interleaved(dec), interleaved(rec)
        say(f"{kind} {wname} level {level}, {K} items of {n} samples of {inner} elements ({vol * esize / 1e6:.1f} MB per band)")
        for name in dec:
            say(f"    {name:52s} dec {td[name][0]:10.1f} us [{td[name][1]:.1f} .. {td[name][2]:.1f}]   rec {tr[name][0]:10.1f} us [{tr[name][1]:.1f} .. {tr[name][2]:.1f}]")
        say(json.dumps({"shape": shape, "level": level, "wname": wname, "bytes_per_band": vol * esize,
                        "lines": {nm: {"dec_us": round(td[nm][0], 1), "rec_us": round(tr[nm][0], 1)} for nm in dec}}))
        pa.close()
        del x, y, out_x, out_y, plans, dec, rec
        torch.cuda.empty_cache()

if args.controls and not parent_lib:
    say("unbatched controls SKIPPED: they compare this build with the parent's and need --parent-lib")
for control in [v for v in args.controls.split(",") if v and parent_lib]:
    kind, dd = control.split(":")
    sizes = [int(v) for v in dd.split("x")]
    if kind == "many":                                        # a batched 1-D plan: K signals of N floats
        rdt, cplx, dims, howmany, n = torch.float32, False, [sizes[1]], sizes[0], sizes[0] * sizes[1]
    else:
        rdt, cplx = KINDS[kind]
        dims, howmany, n = list(reversed(sizes)), None, (2 if cplx else 1)
        for d in dims:
            n *= d
    nb = int(ndwt.num_bands(len(dims), level))
    x = torch.randn(n, dtype=rdt, device="cuda")
    y = torch.randn(nb * n, dtype=rdt, device="cuda")
    out_y, out_x = torch.empty_like(y), torch.empty_like(x)
    pl = {"parent": RawPlan(parent_lib, dims, rdt, cplx, "db4", howmany), "this build": RawPlan(this_lib, dims, rdt, cplx, "db4", howmany)}
    td = interleaved({k: (lambda p=p: p.dec(x.data_ptr(), out_y.data_ptr())) for k, p in pl.items()}, rounds=10, per_round=10)
    tr = interleaved({k: (lambda p=p: p.rec(y.data_ptr(), out_x.data_ptr())) for k, p in pl.items()}, rounds=10, per_round=10)
    say(f"control {control}, db4 level {level}:")
    for k in pl:
        say(f"    {k:12s} dec {td[k][0]:9.1f} us [{td[k][1]:.1f} .. {td[k][2]:.1f}]   rec {tr[k][0]:9.1f} us [{tr[k][1]:.1f} .. {tr[k][2]:.1f}]")
    say(f"    this build / parent: dec {td['this build'][0] / td['parent'][0]:.4f}, rec {tr['this build'][0] / tr['parent'][0]:.4f}")
    say(json.dumps({"control": control, "dec_us": {k: round(td[k][0], 1) for k in pl}, "rec_us": {k: round(tr[k][0], 1) for k in pl}}))
    for p in pl.values():
        p.close()
