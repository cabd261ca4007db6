"""The two BVH builders on the headline scene (bench.py's 1M triangles plus floor, 512x512 at 64 spp):
the host's binned-SAH build (drt_scene_build, tree-identical to the reference) against the device LBVH
(drt_build_bvh_device) committed by the host, and the same LBVH committed on the device
(drt_build_bvh_device_commit) with and without installing the tree in the host scene; the headline frame on
each committed tree.  The PLOC builder (drt_build_bvh_device_ex, build="ploc") is two more arms, ploc (host commit)
and ploc_dcommit (device commit), with its round count, and the builds line carries each tree's surface-area
cost: (sum of inner box surfaces + sum of leaf box surfaces x objects) / the root's surface.  The binned-SAH
builder (build="binned", the host's tree built on the device) is three more arms: binned, binned_dcommit and
binned_dcommit_noinstall, with its level-wise round count.

Two JSON lines:
  builds  --rounds interleaved rounds after one warm-up round, each on a fresh Scene: the host build's ms
          (host clock around drt_scene_build) and the device build's three drt_bvh_build_info times (HIP
          events around the kernels and around the fetch, host clock around the drt_upload_bvh commit — HIP
          events around the commit kernels in the dcommit arms), plus the host clock around each whole upload
          call; arms: device (host commit), dcommit (device commit), dcommit_noinstall (install=False);
  frames  one context per arm in one process, alternating frame by frame: device ms of the frame
          (HIP events), Mrays/s = (closest + shadow traversals of a stats frame) / median ms, the
          shadow-query stream's ms (drt_frame_stage_times) and the binary tree's depth.

  python tools/bvh_build_ab.py [--rounds 10] [--tris 1000000] > profiles/gpu_bvh_ploc.jsonl
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


def tree_depth(tree):
    """depth of an exported tree (root = 1), level by level"""
    level, depth = np.zeros(1, np.int64), 0
    while len(level):
        depth += 1
        inner = level[tree["leaf"][level] == 0]
        left = tree["index"][inner].astype(np.int64)
        level = np.concatenate([left, left + 1])
    return depth


def sa_cost(tree):
    e = tree["boxes"][:, 3:].astype(np.float64) - tree["boxes"][:, :3]
    area = e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2] + e[:, 2] * e[:, 0]
    leaf = tree["leaf"].astype(bool)
    return round(float((area[~leaf].sum() + (area[leaf] * tree["nobjs"][leaf]).sum()) / area[0]), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--ploc-radius", type=int, default=8, help="kPlocRadius of the library under test (a label)")
    args = ap.parse_args()
    tris = bench.synthetic_triangles(args.tris)

    def fresh():
        s = drt.Scene()
        bench.populate(s, tris, args.res, args.spp)
        return s

    dev_arms = {"device": {}, "dcommit": {"commit": "device"}, "dcommit_noinstall": {"commit": "device", "install": False},
                "ploc": {"build": "ploc"}, "ploc_dcommit": {"build": "ploc", "commit": "device"},
                "binned": {"build": "binned"}, "binned_dcommit": {"build": "binned", "commit": "device"},
                "binned_dcommit_noinstall": {"build": "binned", "commit": "device", "install": False}}
    ctx = {a: drt.Renderer(0) for a in ("host", *dev_arms)}
    rows = {"host_build_ms": [], "host_upload_wall_ms": []}
    rows.update({f"{a}_{k}_ms": [] for a in dev_arms for k in ("build", "fetch", "commit", "upload_wall")})
    scenes = {}
    for rnd in range(args.rounds + 1):  # round 0 warms both arms up (code objects, allocations, pinned buffers)
        s = fresh()
        t0 = time.perf_counter()
        s.build()
        t1 = time.perf_counter()
        ctx["host"].upload(s)
        t2 = time.perf_counter()
        scenes = {"host": s}
        if rnd:
            rows["host_build_ms"].append((t1 - t0) * 1e3)
            rows["host_upload_wall_ms"].append((t2 - t0) * 1e3)
        for a, kw in dev_arms.items():
            d = fresh()
            t3 = time.perf_counter()
            ctx[a].upload(d, **{"build": "device", **kw})
            t4 = time.perf_counter()
            scenes[a] = d
            if rnd == 0:
                continue
            bi = ctx[a].bvh_build_info()
            for k in ("build", "fetch", "commit"):
                rows[f"{a}_{k}_ms"].append(bi[f"{k}_ms"])
            rows[f"{a}_upload_wall_ms"].append((t4 - t3) * 1e3)
    out = {"record": "builds", "objects": int(scenes["host"].info().n_objects), "rounds": args.rounds}
    out.update({k: spread(v) for k, v in rows.items()})
    out["host_build_over_device_build_plus_fetch"] = round(
        out["host_build_ms"]["median"] / (out["device_build_ms"]["median"] + out["device_fetch_ms"]["median"]), 1)
    out["commit_info"] = {a: ctx[a].bvh_commit_info() for a in dev_arms}
    out["ploc_rounds"] = {k: ctx["ploc"].bvh_build_info()[k] for k in ("rounds", "forced_rounds")}
    out["ploc_radius"] = args.ploc_radius
    out["binned_rounds"] = ctx["binned"].bvh_build_info()["rounds"]
    out["sa_cost"] = {a: sa_cost(scenes[a].bvh_export()) for a in ("host", "device", "ploc", "binned")}
    print(json.dumps(out), flush=True)

    arms = tuple(ctx)
    rays, ms, stream = {}, {a: [] for a in arms}, {a: [] for a in arms}
    for a in arms:
        ctx[a].render(seed=7, stats=True)
        st = ctx[a].stats()
        rays[a] = st["closest_rays"] + st["shadow_rays"]
    for rnd in range(args.rounds + 2):  # two warm-up rounds
        for a in arms:
            ctx[a].render(seed=7)
            if rnd >= 2:
                ms[a].append(float(ctx[a].frame_times(1)[1][-1]))
                try:
                    stream[a].append(float(ctx[a].frame_stage_times()["stream"]))
                except RuntimeError:  # not a wavefront frame: no shadow-query stream to time
                    stream[a].append(float("nan"))
    out = {"record": "frames", "res": args.res, "spp": args.spp, "rounds": args.rounds}
    for a in arms:
        m = spread(ms[a])
        out[a] = {"frame_ms": m, "mrays_s": round(rays[a] / m["median"] / 1e3, 1), "rays": int(rays[a]),
                  "trace_stream_ms": spread(stream[a])}
        if a == "host":
            out[a].update(bvh_depth=tree_depth(scenes[a].bvh_export()), bvh_nodes=int(scenes[a].info().bvh_nodes))
        else:  # (a scene without the tree installed has none to export)
            bi = ctx[a].bvh_build_info()
            out[a].update(bvh_depth=bi["depth"], bvh_nodes=bi["n_nodes"])
    for a in dev_arms:
        out[f"{a}_over_host_frame_rate"] = round(out["host"]["frame_ms"]["median"] / out[a]["frame_ms"]["median"], 3)
    out["dcommit_over_device_frame_rate"] = round(
        out["device"]["frame_ms"]["median"] / out["dcommit"]["frame_ms"]["median"], 3)
    out["ploc_over_device_frame_rate"] = round(out["device"]["frame_ms"]["median"] / out["ploc"]["frame_ms"]["median"], 3)
    out["ploc_radius"] = args.ploc_radius
    out["binned_over_ploc_frame_rate"] = round(out["ploc"]["frame_ms"]["median"] / out["binned"]["frame_ms"]["median"], 3)
    print(json.dumps(out), flush=True)
    for r in ctx.values():
        r.close()


if __name__ == "__main__":
    main()
