"""Interleaved A/B of whole frames: a mixed-primitive Grid scene's shadow queries on the Grid walk
(DRT_GRID_CELL_TREE=0, arm "walk": grid_stream, what the scene ran before the cell tree) against the
cell tree (DRT_GRID_CELL_TREE=1, arm "tree": cell_tree_stream + the walk for the undecided queries).

Both arms run in one process on one upload, alternating frame by frame (the knob is read per frame), in
the scene's own frame mode (Whitted) and as a 16-spp AA frame.  Rays = closest + shadow traversals of a
stats frame, Mrays/s = rays / median device ms of the frame (path kernels + reduce, HIP events).  One
JSON line per (scene, mode), with the share of shadow queries the tree sent to the walk and whether the
two arms' frames are bit-identical.

  python tools/cell_tree_ab.py [--rounds 40] > profiles/grid_cell_tree_ab.jsonl
"""
import argparse
import json
import os
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import distributionraytracer_amd as drt  # noqa: E402
import shipped  # noqa: E402


def frame(r, arm, **kw):
    os.environ["DRT_GRID_CELL_TREE"] = "1" if arm == "tree" else "0"
    return r.render(seed=7, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--scenes", default="balls_high,assignment1")
    args = ap.parse_args()
    os.environ["DRT_GRID_CELL_TREE"] = "1"  # the upload builds the tree
    r = drt.Renderer(0)
    with tempfile.TemporaryDirectory() as tmp:
        for name in args.scenes.split(","):
            for mode, spp in (("whitted", None), ("aa16", 16)):
                d = Path(tmp) / f"{name}_{mode}"
                d.mkdir()
                over = {"accel": "grid"} if spp is None else {"accel": "grid", "spp": spp}
                s = drt.Scene.load_p3f(shipped.write(d, name, **over), skybox_faces=shipped.skybox_faces(name))
                s.build()
                r.upload(s)
                plan = r.plan(r.frame_params(seed=7))
                frame(r, "walk", stats=True)
                st = r.stats()
                rays = st["closest_rays"] + st["shadow_rays"]
                os.environ["DRT_GRID_SHADOW_TREE"] = "2"  # a stats frame on the tree
                frame(r, "tree", stats=True)
                tst = r.stats()
                del os.environ["DRT_GRID_SHADOW_TREE"]
                imgs = {arm: frame(r, arm) for arm in ("walk", "tree")}
                for _ in range(3):
                    for arm in ("walk", "tree"):
                        frame(r, arm)
                for _ in range(args.rounds):
                    for arm in ("walk", "tree"):
                        frame(r, arm)
                _, ms = r.frame_times(2 * args.rounds)
                ms = ms[-2 * args.rounds:]
                out = {"scene": name, "mode": mode, "objects": int(s.info().n_objects), "passes": plan["passes"],
                       "wavefront": plan["wavefront"], "rays": int(rays), "rounds": args.rounds}
                for k, arm in enumerate(("walk", "tree")):
                    a = ms[k::2]
                    out[arm] = {"ms_median": round(float(np.median(a)), 4), "ms_min": round(float(a.min()), 4),
                                "ms_p90": round(float(np.percentile(a, 90)), 4),
                                "mrays_s": round(rays / float(np.median(a)) / 1e3, 1)}
                out["tree_over_walk"] = round(out["walk"]["ms_median"] / out["tree"]["ms_median"], 3)
                out["shadow_rays"] = int(tst["shadow_rays"])
                out["tree_queries"] = int(tst["wide_shadow_rays"])
                out["walked_share"] = round(tst["wide_grid_walks"] / max(1, tst["shadow_rays"]), 5)
                out["tree_tests_per_query"] = round((tst["wide_inner"] + tst["wide_prims"]) / max(1, tst["wide_shadow_rays"]), 2)
                out["walk_tests_per_query"] = round(st["shadow_prims"] / max(1, st["shadow_rays"]), 2)
                out["frames_identical"] = bool(np.array_equal(imgs["walk"].view(np.uint32), imgs["tree"].view(np.uint32)))
                print(json.dumps(out), flush=True)
    r.close()


if __name__ == "__main__":
    main()
