"""One rank's share of an 8-rank cfg5 run (256^3 x 32, db4, 3 levels, fp32), measured on one GPU at world size 1 for both
decompositions of ShardedNdDwt: t-slabs (256^3 x 4 frames) and z-slabs (256 x 256 x 32 planes x 32 frames).  Every exchange
segment is a copy on the rank itself (the compute side and the local halo traffic, "before communication"); the halo bytes per
level and rank that an 8-rank run would move between GPUs are computed from the halo planes.  No multi-GPU run is involved.

usage: python tools/zshard_one_rank.py [steps] [--json out.json]
"""
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import importlib  # noqa: E402

sh = importlib.import_module("non-decimated_wavelets_amd.sharded")

N, NT, RANKS, WN, LEVEL = 256, 32, 8, "db4", 3


def measure(sizes, shard_axis, global_len, steps):
    dev = torch.device("cuda", 0)
    local = list(sizes)
    eng = sh.HipSlabEngine([WN] * 4, local, torch.float32, True, "reference", dev, global_outer=global_len,
                           shard_axis=shard_axis if shard_axis != 3 else None)
    drv = sh.ShardedNdDwt(WN, sizes, pres_l2_norm=True, precision="single", device=dev, engine=eng, overlap=False,
                          shard_axis=shard_axis if shard_axis != 3 else None)
    torch.manual_seed(0)
    x = torch.randn(*reversed(sizes), device=dev)
    for _ in range(3):
        drv.rec(drv.dec(x, LEVEL))
    torch.cuda.synchronize()
    gc.collect()
    gc.freeze()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    dec_ms, rec_ms = [], []
    t0 = time.perf_counter()
    for _ in range(steps):
        ev[0].record()
        y = drv.dec(x, LEVEL)
        ev[1].record()
        r = drv.rec(y)
        ev[2].record()
        ev[2].synchronize()
        dec_ms.append(ev[0].elapsed_time(ev[1]))
        rec_ms.append(ev[1].elapsed_time(ev[2]))
    wall = (time.perf_counter() - t0) / steps * 1e3
    gc.unfreeze()
    err = float((r - x).abs().max())
    ab, aa, sb, sa = eng.halo(1)
    plane = 4 * N * N                                            # bytes of one (ny, nx) plane, fp32
    frames = sizes[3] if shard_axis == 2 else 1
    per_plane = plane * (N if shard_axis == 3 else 1) * frames   # t-slab: a plane of the sharded axis is a whole 256^3 frame
    med = lambda v: sorted(v)[len(v) // 2]
    return {
        "local_sizes": sizes, "shard_axis": shard_axis, "scheme": drv.scheme,
        "ms_dec_median": round(med(dec_ms), 3), "ms_rec_median": round(med(rec_ms), 3),
        "ms_step_median": round(med([a + b for a, b in zip(dec_ms, rec_ms)]), 3), "ms_step_wall": round(wall, 3),
        "halo_MiB_per_level_and_rank_analysis": (ab + aa) * per_plane / 2 ** 20,
        "halo_MiB_per_level_and_rank_synthesis_scatter": (sb + sa) * per_plane / 2 ** 20,
        "roundtrip_max_abs_err": err,
    }


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else 20
    out = {
        "what": "one rank's share of an 8-rank cfg5 run (256^3 x 32, db4, 3 levels, fp32) on ONE MI355X at world size 1",
        "note": "every exchange segment is a copy on the rank itself; the halo bytes are those an 8-rank run would move per level and "
                "rank; no multi-GPU run has been measured",
        "device": torch.cuda.get_device_name(0),
        "steps": steps,
        # t-slab: 4 frames of 32 (the slab plan's length check is on the whole t axis); z-slab: 32 planes of 256, all 32 frames
        "t_slab": measure([N, N, N, NT // RANKS], 3, NT, steps),
        "z_slab": measure([N, N, N // RANKS, NT], 2, N, steps),
    }
    out["halo_ratio_t_over_z"] = out["t_slab"]["halo_MiB_per_level_and_rank_analysis"] / out["z_slab"]["halo_MiB_per_level_and_rank_analysis"]
    txt = json.dumps(out, indent=1)
    print(txt)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
