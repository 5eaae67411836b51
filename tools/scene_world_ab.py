"""Wall time of the three ways to change a scene with constant media on one GPU:

  (a) re-create   rrt_scene_destroy + rrt_scene_create_ex with RRT_FLAG_DEVICE_BVH of the new inputs,
                  the only way before rrt_scene_update_world existed (`--arm recreate`; run it on
                  the parent's library with RRT_LIB_PATH to time the parent itself);
  (b) update      rrt_scene_update_world on the scene that is kept: the media classified again on the
                  host, a rebuild on the device;
  (c) refit       rrt_scene_refit_world on a scene that is kept, as the enqueue-to-event time (two
                  events on the stream around the call, read after a synchronisation) beside the wall
                  time the call blocks the calling thread.

Scenes: `NW9` (the_next_week 9, final_scene: 1006 spheres, 2401 quads, 2 sphere media, one of them
tested outside the tree) and `NW8` (the_next_week 8, cornell_smoke: 6 quads, 2 box media, 12 boundary
quads). Every set moves all of it: seeded jitters of the spheres, the quads, the media's spheres and
densities and each medium's boundary as a whole. One warm-up per arm (the first update and the first
refit allocate), then `--rounds` rounds, every round printed, then median (min-max) and one JSON line
per scene. All arms go through the Python wrappers, whose own cost is part of every wall-time figure.

    python tools/scene_world_ab.py [--arm all|recreate] [--scenes NW9,NW8] [--rounds 9]
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stat(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
            "n": len(v)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--arm", default="all", choices=("all", "recreate"))
    ap.add_argument("--scenes", default="NW9,NW8")
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()

    import numpy as np
    import torch

    import rustraytrace_amd as rrt

    if not torch.cuda.is_available() or rrt.device_count() < 1:
        raise SystemExit("scene_world_ab: no HIP device (this is a measurement: it does not run without one)")

    def scene_of(name):
        if name in ("NW8", "NW9"):
            return rrt.next_week_scene(int(name[2:]), dict(image_width=32, samples_per_pixel=4))
        raise SystemExit(f"scene_world_ab: unknown scene {name!r}")

    def moved(sc, rng, amount=0.01):
        sp = sc.spheres.copy()
        r = np.maximum(sp["center_radius"][:, 3:4], 0.0)
        sp["center_radius"][:, :3] += (rng.normal(0.0, amount, (len(sp), 3)) * np.minimum(r, 10.0)).astype(np.float32)
        q = sc.quads.copy()
        ext = np.maximum(np.linalg.norm(q["u"][:, :3], axis=1), np.linalg.norm(q["v"][:, :3], axis=1))[:, None]
        for k in ("q", "u", "v"):
            q[k][:, :3] += (rng.normal(0.0, amount, (len(q), 3)) * ext).astype(np.float32)
        md = sc.media.copy()
        bq = None if sc.boundary_quads is None else sc.boundary_quads.copy()
        for m in range(len(md)):
            md["density"][m] *= np.float32(1.0 + 0.5 * amount * rng.uniform(-1.0, 1.0))
            if int(md["boundary_kind"][m]) == 0:
                md["sphere"][m, :3] += (rng.normal(0.0, amount, 3) * min(float(md["sphere"][m, 3]), 10.0)).astype(np.float32)
            else:
                rows = slice(int(md["first"][m]), int(md["first"][m]) + int(md["count"][m]))
                size = np.linalg.norm(bq["u"][rows, :3], axis=1).max()
                bq["q"][rows, :3] += (rng.normal(0.0, amount, 3) * size).astype(np.float32)
        return dataclasses.replace(sc, spheres=sp, quads=q, media=md, boundary_quads=bq)

    def change(ds, how, new, **kw):
        getattr(ds, how)(spheres=new.spheres, motion=new.motion, quads=new.quads, media=new.media,
                         boundary_quads=new.boundary_quads, **kw)

    stream = torch.cuda.current_stream()
    for name in args.scenes.split(","):
        sc = scene_of(name)
        rng = np.random.default_rng(2024)
        scenes = [moved(sc, rng) for _ in range(8)]
        line = {"tool": "scene_world_ab", "arm": args.arm, "scene": name, "spheres": len(sc.spheres), "quads": len(sc.quads),
                "media": len(sc.media), "boundary_quads": 0 if sc.boundary_quads is None else len(sc.boundary_quads),
                "library": os.environ.get("RRT_LIB_PATH", "this build")}
        ms = {"recreate": [], "update": [], "refit_event": [], "refit_blocked": []}
        again = rrt.DeviceScene(sc, device=0, device_bvh=True)  # warm-up of (a)
        if args.arm == "all":
            kept = rrt.DeviceScene(sc, device=0, device_bvh=True)
            change(kept, "update_world", scenes[0])  # warm-up of (b)
            fitted = rrt.DeviceScene(sc, device=0, device_bvh=True)
            change(fitted, "refit_world", scenes[0], stream_ptr=stream.cuda_stream)  # warm-up of (c)
            torch.cuda.synchronize()
        for r in range(args.rounds):
            k = (r + 1) % len(scenes)
            torch.cuda.synchronize()
            t = time.perf_counter()
            again.close()
            again = rrt.DeviceScene(scenes[k], device=0, device_bvh=True)
            ms["recreate"].append((time.perf_counter() - t) * 1e3)
            if args.arm == "all":
                t = time.perf_counter()
                change(kept, "update_world", scenes[k])
                ms["update"].append((time.perf_counter() - t) * 1e3)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                t = time.perf_counter()
                change(fitted, "refit_world", scenes[k], stream_ptr=stream.cuda_stream)
                ms["refit_blocked"].append((time.perf_counter() - t) * 1e3)
                e1.record(stream)
                torch.cuda.synchronize()
                ms["refit_event"].append(e0.elapsed_time(e1))
                assert kept.update_stats()["last_allocations"] == 0 and fitted.refit_stats()["last_allocations"] == 0
            print(f"{name} round {r}: " + "  ".join(f"{k2} {v[-1]:.3f} ms" for k2, v in ms.items() if v), flush=True)
        again.close()
        for k2, v in ms.items():
            if v:
                line[k2] = stat(v)
        if args.arm == "all":
            line["tree"] = {k2: v for k2, v in kept.bvh_info().items() if k2 in ("n_nodes", "max_depth", "node_stride", "n_unbounded")}
            line["refit_launches"] = fitted.refit_stats()["last_launches"]
            kept.close()
            fitted.close()
        print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
