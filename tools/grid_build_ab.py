"""The host and the device grid builders on the Grid headline scene (bench.py's 1M triangles plus floor,
512x512 at 64 spp): drt_scene_build + drt_scene_upload against drt_build_grid_device committed by the host
(drt_upload_grid), committed on the device, and committed on the device without installing the lists in the
host scene; the headline frame on the host path's grid (shadow tree) and on the device-built grid (Grid walk).

Two JSON lines, every figure as median [min, max]:
  builds  --rounds interleaved rounds after one warm-up round, each on a fresh Scene.  Host arm: Grid::Build
          alone (drt_scene_info's build_ms, host clock), the BVH built for the shadow tree (host clock around
          drt_scene_build minus Grid::Build) and the whole build + upload call.  Device arms: the three
          drt_grid_build_info times (HIP events around the build kernels; around the fetch; host clock around
          drt_upload_grid — which is the host's commit, measured alone — or HIP events around the commit
          kernels) and the host clock around each whole upload call.
  frames  one context per arm in one process, alternating frame by frame: device ms of the frame (HIP
          events) and Mrays/s = (closest + shadow traversals of a stats frame) / median ms.

  python tools/grid_build_ab.py [--rounds 10] [--tris 1000000] > profiles/gpu_grid_build.jsonl

--shadow-trees adds two device arms whose upload also builds and commits the Grid scene's shadow tree on the
device (shadow_tree="device": LBVH, "ploc": PLOC; commit="device"): their builds record carries the tree's
builder and commit times (drt_bvh_build_info, HIP events), their frames answer shadow queries on that tree.

  python tools/grid_build_ab.py --shadow-trees --rounds 5 > profiles/gpu_grid_shadow_build.jsonl
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402
import distributionraytracer_amd as drt  # noqa: E402


def spread(a):
    a = np.asarray(a, np.float64)
    return {"median": round(float(np.median(a)), 3), "min": round(float(a.min()), 3), "max": round(float(a.max()), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--shadow-trees", action="store_true")
    args = ap.parse_args()
    tris = bench.synthetic_triangles(args.tris)

    def fresh():
        s = drt.Scene()
        bench.populate(s, tris, args.res, args.spp, accel="grid")
        return s

    dev_arms = {"device": {}, "dcommit": {"commit": "device"}, "dcommit_noinstall": {"commit": "device", "install": False}}
    tree_arms = {"dcommit_lbvh": "device", "dcommit_ploc": "ploc"} if args.shadow_trees else {}
    dev_arms.update({a: {"commit": "device", "shadow_tree": t} for a, t in tree_arms.items()})
    ctx = {a: drt.Renderer(0) for a in ("host", *dev_arms)}
    rows = {"host_grid_build_ms": [], "host_shadow_bvh_build_ms": [], "host_upload_wall_ms": []}
    rows.update({f"{a}_{k}_ms": [] for a in dev_arms for k in ("build", "fetch", "commit", "upload_wall")})
    rows.update({f"{a}_shadow_{k}_ms": [] for a in tree_arms for k in ("build", "commit")})
    info = None
    for rnd in range(args.rounds + 1):  # round 0 warms every arm up (code objects, allocations, pinned buffers)
        s = fresh()
        t0 = time.perf_counter()
        s.build()
        t1 = time.perf_counter()
        ctx["host"].upload(s)
        t2 = time.perf_counter()
        if rnd:
            grid_ms = float(s.info().build_ms)
            rows["host_grid_build_ms"].append(grid_ms)
            rows["host_shadow_bvh_build_ms"].append((t1 - t0) * 1e3 - grid_ms)
            rows["host_upload_wall_ms"].append((t2 - t0) * 1e3)
        for a, kw in dev_arms.items():
            d = fresh()
            t3 = time.perf_counter()
            ctx[a].upload(d, build="device", **kw)
            t4 = time.perf_counter()
            if rnd == 0:
                continue
            info = ctx[a].grid_build_info()
            for k in ("build", "fetch", "commit"):
                rows[f"{a}_{k}_ms"].append(info[f"{k}_ms"])
            rows[f"{a}_upload_wall_ms"].append((t4 - t3) * 1e3)
            if a in tree_arms:
                assert info["shadow_tree"] == (1 if tree_arms[a] == "device" else 2), info
                tree = ctx[a].bvh_build_info()
                rows[f"{a}_shadow_build_ms"].append(tree["build_ms"])
                rows[f"{a}_shadow_commit_ms"].append(tree["commit_ms"])
    out = {"record": "builds", "objects": int(s.info().n_objects), "rounds": args.rounds, "dims": info["dims"],
           "n_cells": info["n_cells"], "n_refs": info["n_refs"]}
    out.update({k: spread(v) for k, v in rows.items()})
    out["host_drt_upload_grid_ms"] = out["device_commit_ms"]  # the same function on the same lists
    for a in dev_arms:
        out[f"host_over_{a}_upload_wall"] = round(
            out["host_upload_wall_ms"]["median"] / out[f"{a}_upload_wall_ms"]["median"], 1)
    print(json.dumps(out), flush=True)

    arms = ("host", "dcommit", *tree_arms)
    rays, ms = {}, {a: [] for a in arms}
    for a in arms:
        ctx[a].render(seed=7, stats=True)
        st = ctx[a].stats()
        rays[a] = st["closest_rays"] + st["shadow_rays"]
    for rnd in range(args.rounds + 2):  # two warm-up rounds
        for a in arms:
            ctx[a].render(seed=7)
            if rnd >= 2:
                ms[a].append(float(ctx[a].frame_times(1)[1][-1]))
    out = {"record": "frames", "res": args.res, "spp": args.spp, "rounds": args.rounds,
           "shadow_queries": {"host": "shadow tree", "dcommit": "Grid walk",
                              **{a: f"device-built shadow tree ({t})" for a, t in tree_arms.items()}}}
    for a in arms:
        m = spread(ms[a])
        out[a] = {"frame_ms": m, "mrays_s": round(rays[a] / m["median"] / 1e3, 1), "rays": int(rays[a])}
    for a in arms[1:]:
        out[f"{a}_over_host_frame_rate"] = round(out["host"]["frame_ms"]["median"] / out[a]["frame_ms"]["median"], 3)
    print(json.dumps(out), flush=True)
    for r in ctx.values():
        r.close()


if __name__ == "__main__":
    main()
