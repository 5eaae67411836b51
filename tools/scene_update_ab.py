"""A/B of the two ways to change a scene's spheres on one GPU, in one process:

  (a) re-create   rrt_scene_destroy + rrt_scene_create_ex with RRT_FLAG_DEVICE_BVH — the only way
                  before rrt_scene_update_spheres existed;
  (b) update      rrt_scene_update_spheres on the scene that is kept.

  change     wall-clock of one change of the spheres, (a) against (b), in interleaved rounds after one
             warm-up each (the warm-up of (b) is the scene's first update, which allocates); every round
             is printed, then median (min-max). Both arms go through the Python wrappers (DeviceScene,
             DeviceScene.update_spheres), whose own cost is part of either figure.
  loop       `--frames` frames at `--width` x `--spp` that move the spheres before every frame and render
             it on one stream, timed as a whole (wall-clock until the last frame is done), both ways.

    python tools/scene_update_ab.py [--scenes C2,NW1,C5,G160] [--rounds 7] [--width 480] [--spp 16] [--frames 16]

G160 is the RTOW scene with grid_half = 160 (about 10^5 spheres). The sphere sets are seeded jitters of
the scene's centers (NW1 keeps its motion rows). One JSON line per scene at the end.
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
    ap.add_argument("--scenes", default="C2,NW1,C5,G160")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--frames", type=int, default=16)
    args = ap.parse_args()

    import numpy as np
    import torch

    import rustraytrace_amd as rrt

    if not torch.cuda.is_available() or rrt.device_count() < 1:
        raise SystemExit("scene_update_ab: no HIP device (this is a measurement: it does not run without one)")

    def scene_of(name):
        kw = dict(image_width=args.width, samples_per_pixel=args.spp)
        if name == "G160":
            return rrt.rtow(grid_half=160, max_depth=50, **kw)
        return rrt.named_scene(name, **kw)

    stream = torch.cuda.current_stream()
    for name in args.scenes.split(","):
        sc = scene_of(name)
        rng = np.random.default_rng(2024)
        sets = []
        for _ in range(8):
            sp = sc.spheres.copy()
            sp["center_radius"][:, :3] += rng.normal(0.0, 0.05, (len(sp), 3)).astype(np.float32)
            sets.append(sp)
        scenes = [dataclasses.replace(sc, spheres=sp) for sp in sets]
        line = {"tool": "scene_update_ab", "scene": name, "spheres": len(sc.spheres), "image": [sc.width, sc.height],
                "spp": sc.spp}

        # ---- one change ----
        kept = rrt.DeviceScene(sc, device=0, device_bvh=True)
        kept.update_spheres(sets[0], sc.motion)  # warm-up of (b): the first update allocates
        line["first_update"] = kept.update_stats()
        again = rrt.DeviceScene(sc, device=0, device_bvh=True)  # warm-up of (a)
        ms = {"recreate": [], "update": []}
        for r in range(args.rounds):
            k = (r + 1) % len(sets)
            t = time.perf_counter()
            again.close()
            again = rrt.DeviceScene(scenes[k], device=0, device_bvh=True)
            ms["recreate"].append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            kept.update_spheres(sets[k], sc.motion)
            ms["update"].append((time.perf_counter() - t) * 1e3)
            print(f"{name} change round {r}: re-create {ms['recreate'][-1]:.3f} ms  update {ms['update'][-1]:.3f} ms",
                  flush=True)
        line["steady_update"] = kept.update_stats()
        line["tree"] = {k: v for k, v in kept.bvh_info().items() if k in ("n_nodes", "max_depth", "node_stride")}
        line["recreate"] = stat(ms["recreate"])
        line["update"] = stat(ms["update"])
        line["update_median_below_recreate_min"] = statistics.median(ms["update"]) < min(ms["recreate"])
        line["speedup"] = round(statistics.median(ms["recreate"]) / statistics.median(ms["update"]), 2)
        again.close()

        # ---- the frame loop ----
        tile = kept.tile(16, 0, 1, 0, sc.spp)
        buf = torch.empty((sc.height, sc.width, 4), dtype=torch.float32, device="cuda:0")
        kept.render_tile_async(tile, buf.data_ptr(), stream.cuda_stream)  # warm-up frame
        torch.cuda.synchronize()
        loops = {"recreate": [], "update": []}
        for r in range(3):
            ds = rrt.DeviceScene(sc, device=0, device_bvh=True)
            t = time.perf_counter()
            for f in range(args.frames):
                torch.cuda.synchronize()  # the scene being destroyed must not be in use
                ds.close()
                ds = rrt.DeviceScene(scenes[f % len(sets)], device=0, device_bvh=True)
                ds.render_tile_async(tile, buf.data_ptr(), stream.cuda_stream)
            torch.cuda.synchronize()
            loops["recreate"].append((time.perf_counter() - t) * 1e3)
            ds.close()
            t = time.perf_counter()
            for f in range(args.frames):
                kept.update_spheres(sets[f % len(sets)], sc.motion, stream_ptr=stream.cuda_stream)
                kept.render_tile_async(tile, buf.data_ptr(), stream.cuda_stream)
            torch.cuda.synchronize()
            loops["update"].append((time.perf_counter() - t) * 1e3)
            print(f"{name} {args.frames}-frame loop round {r}: re-create {loops['recreate'][-1]:.2f} ms  "
                  f"update {loops['update'][-1]:.2f} ms", flush=True)
        kept.close()
        line["loop_frames"] = args.frames
        line["loop_recreate"] = stat(loops["recreate"])
        line["loop_update"] = stat(loops["update"])
        print(f"{name}: re-create {line['recreate']['median_ms']} ({line['recreate']['min_ms']}-{line['recreate']['max_ms']}) ms, "
              f"update {line['update']['median_ms']} ({line['update']['min_ms']}-{line['update']['max_ms']}) ms", flush=True)
        print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
