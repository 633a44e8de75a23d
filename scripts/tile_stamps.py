"""Developer probe (GPU box): where the workgroups of the headline render's two network launches end.

Builds the library with -DDN_TILE_STAMP into a scratch directory (the shipped library has no stamp), renders the headline image
(bench.py: 400x400 rays, 64+128 samples, D8/W256 x2) back to back for at least 2 s, then reads the stamp records of the last render's
coarse and fine launch: per workgroup s_memrealtime (100 MHz, one clock for the whole chip) and s_memtime (the XCD's own shader clock)
at the top of its first tile and behind its last, HW_REG_XCC_ID and the number of tiles it ran.  Reports per XCD the mean and the
latest end, the in-kernel clock (d s_memtime / d s_memrealtime x 100 MHz) and the idle share of the launch:
sum over workgroups of (launch end - own end) / (workgroups x duration).

    python scripts/tile_stamps.py --build-only                       # no GPU needed: cross-compile the stamp library
    python scripts/tile_stamps.py [--src TREE] [--tag NAME] [--json OUT.json] [--precision bf16|fp16] [--repeats N]

--src TREE builds / measures another checkout's dex-nerf_amd/csrc (it must have the switch) - e.g. before and after a scheduling change.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS, MAX_WGS, LAUNCHES = 8, 1024, 4     # mlp_geo48.h kTileStampWords / kTileStampMaxWgs / kTileStampLaunches


def build(src, out_dir):
    lib = os.path.join(out_dir, "libdexnerf_hip.so")
    subprocess.run(["make", "-C", os.path.join(src, "dex-nerf_amd", "csrc"), "-j16", f"BUILD={os.path.join(out_dir, 'build')}", f"OUT={lib}",
                    "EXTRA=-DDN_TILE_STAMP"], check=True)
    return lib


def summarize(rec):
    """rec: [workgroups][8] integers of one launch -> the figures of the report (times in microseconds from the earliest start)."""
    import numpy as np
    rec = np.asarray(rec, dtype=np.int64)
    t0, c0, t1, c1, xcc, tiles = (rec[:, i] for i in range(6))
    start = t0.min()
    end = t1.max()
    dur = float(end - start) / 100.0                       # us
    own_end = (t1 - start) / 100.0
    own_start = (t0 - start) / 100.0
    clock = (c1 - c0) / np.maximum(t1 - t0, 1) * 100.0      # MHz
    out = {"workgroups": int(rec.shape[0]), "n_tiles": int(rec[0, 7]), "tiles_per_workgroup": [int(tiles.min()), int(tiles.max())],
           "tiles_total": int(tiles.sum()), "duration_us": dur, "idle_share": float((dur - own_end).sum() / (rec.shape[0] * dur)),
           "start_spread_us": float(own_start.max()), "clock_mhz_median": float(np.median(clock)), "xcd": []}
    for x in sorted(set(xcc.tolist())):
        m = xcc == x
        out["xcd"].append({"xcc_id": int(x), "workgroups": int(m.sum()), "tiles": int(tiles[m].sum()), "end_mean_us": float(own_end[m].mean()),
                           "end_first_us": float(own_end[m].min()), "end_last_us": float(own_end[m].max()),
                           "idle_share": float((dur - own_end[m]).mean() / dur), "clock_mhz": float(np.median(clock[m])),
                           "us_per_tile": float(((t1 - t0)[m] / 100.0 / np.maximum(tiles[m], 1)).mean())})
    return out


def show(name, s):
    print(f"{name}: {s['workgroups']} workgroups, {s['n_tiles']} tiles ({s['tiles_per_workgroup'][0]}-{s['tiles_per_workgroup'][1]} per workgroup, "
          f"{s['tiles_total']} run), {s['duration_us'] / 1e3:.3f} ms, idle share {s['idle_share'] * 100:.2f} %, clock {s['clock_mhz_median']:.0f} MHz, "
          f"starts within {s['start_spread_us']:.1f} us")
    for x in s["xcd"]:
        print(f"   XCD {x['xcc_id']}: {x['workgroups']:3d} wg {x['tiles']:6d} tiles  end mean {x['end_mean_us'] / 1e3:7.3f} first {x['end_first_us'] / 1e3:7.3f} "
              f"last {x['end_last_us'] / 1e3:7.3f} ms  idle {x['idle_share'] * 100:5.2f} %  clock {x['clock_mhz']:6.0f} MHz  {x['us_per_tile']:6.2f} us/tile")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=REPO, help="checkout whose dex-nerf_amd/csrc is built and measured")
    ap.add_argument("--tag", default="tile_stamp", help="scratch directory exp_libs/<tag>")
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--soak", type=float, default=2.0, help="seconds of back-to-back renders before the stamped one")
    ap.add_argument("--repeats", type=int, default=3, help="stamped renders (each after its own soak)")
    ap.add_argument("--json", help="write every figure here")
    args = ap.parse_args()
    out_dir = os.path.join(REPO, "exp_libs", args.tag)
    lib = os.path.join(out_dir, "libdexnerf_hip.so")
    if args.build_only or not os.path.exists(lib):
        lib = build(args.src, out_dir)
    if args.build_only:
        print(lib)
        return
    os.environ["DEXNERF_HIP_LIB"] = lib
    sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "dex-nerf_amd"))
    import numpy as np
    import torch
    import nerf
    from nerf import _hip
    import bench
    handle = _hip.lib()
    read = ctypes.CDLL(lib).dn_tile_stamp_read
    read.restype = ctypes.c_longlong
    read.argtypes = [ctypes.c_void_p]
    dev = torch.device("cuda:0")
    nerf.set_precision(args.precision)
    if args.precision == "bf16":
        nerf.set_render_policy("bf16")
    scene = bench.build_scene(dev, 0)
    buf = np.zeros((LAUNCHES, MAX_WGS, WORDS), dtype=np.uint64)
    props = torch.cuda.get_device_properties(0)
    result = {"device": torch.cuda.get_device_name(0), "arch": getattr(props, "gcnArchName", None), "uuid": str(getattr(props, "uuid", "")),
              "host": os.uname().nodename, "precision": args.precision, "soak_s": args.soak, "runs": []}
    print(f"device {result['device']} {result['arch']} uuid {result['uuid']} on host {result['host']}")
    for rep in range(args.repeats):
        t0 = time.perf_counter()
        n = 0
        while time.perf_counter() - t0 < args.soak:      # back to back: the queue never drains for longer than the glue launches
            for _ in range(8):
                bench.render(*scene)
            torch.cuda.synchronize()
            n += 8
        for _ in range(8):                               # the stamped render is the last of a batch: seven renders queued in front of it
            bench.render(*scene)
        count = read(buf.ctypes.data)                    # (synchronizes)
        if count < 2:
            raise SystemExit("no stamped launches: is this a -DDN_TILE_STAMP build?")
        run = {"renders_before": n}
        for name, idx in (("coarse", count - 2), ("fine", count - 1)):
            rec = buf[idx % LAUNCHES]
            wgs = int(rec[0, 6])
            run[name] = summarize(rec[:wgs].astype(np.int64))
            show(f"[{rep}] {name}", run[name])
        result["runs"].append(run)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
