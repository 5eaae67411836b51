"""A/B of the three ways to change a scene's spheres on one GPU, in one process:

  (a) re-create   rrt_scene_destroy + rrt_scene_create_ex with RRT_FLAG_DEVICE_BVH — the only way
                  before rrt_scene_update_spheres existed;
  (b) update      rrt_scene_update_spheres on the scene that is kept: a rebuild on the device;
  (c) refit       rrt_scene_refit_spheres on a scene that is kept: the last build's topology over the
                  new boxes, enqueued on the stream. Two figures per round: how long the call blocks the
                  calling thread, and the wall-clock until the device has finished it.

  change     wall-clock of one change of the spheres, (a), (b) and (c), in interleaved rounds after one
             warm-up each (the warm-up of (b) is the scene's first update, which allocates); every round
             is printed, then median (min-max). Both arms go through the Python wrappers (DeviceScene,
             DeviceScene.update_spheres), whose own cost is part of either figure.
  loop       `--frames` frames at `--width` x `--spp` that move the spheres before every frame and render
             it on one stream, timed as a whole (wall-clock until the last frame is done), each way; a
             fourth column refits every frame and rebuilds (update) when rrt_scene_tree_cost's
             sah / sah_at_build passes `--rebuild-at` (checked every `--cost-every` frames; the loop's
             sphere sets are a random walk, so the tree does degrade).
  quality    with `--quality`: render time of one frame over a refitted tree against a rebuilt one
             after jitters of scale 0.05, 0.4 and 2.0, beside sah / sah_at_build.
  forms      with `--forms`: the refit's device time with the per-level launches forced against the
             single workgroup forced (rrt_testing_refit_form), on RTOW scenes of growing size (the single
             workgroup is refused past kRefitSmallMaxNodes of rrt_bvh_build.hip: raise it to compare there).

    python tools/scene_update_ab.py [--scenes C2,NW1,C5,G160] [--rounds 7] [--width 480] [--spp 16] [--frames 16]
                                    [--rebuild-at 1.005] [--cost-every 4] [--quality] [--forms]

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
    ap.add_argument("--rebuild-at", type=float, default=1.005, help="loop: rebuild when sah / sah_at_build passes this")
    ap.add_argument("--cost-every", type=int, default=4, help="loop: frames between two looks at the tree's cost")
    ap.add_argument("--quality", action="store_true", help="also: frame time over refitted against rebuilt trees")
    ap.add_argument("--forms", action="store_true", help="only: the two forms of the refit's bottom-up pass by size")
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

    def timed_refit(ds, spheres, motion):
        """(ms the call blocked this thread, ms until the device finished it)."""
        t = time.perf_counter()
        ds.refit_spheres(spheres, motion, stream_ptr=stream.cuda_stream)
        blocked = (time.perf_counter() - t) * 1e3
        torch.cuda.synchronize()
        return blocked, (time.perf_counter() - t) * 1e3

    if args.forms:
        from rustraytrace_amd import _lib

        for grid_half in (4, 8, 11, 16, 22, 32, 45, 64, 90):
            sc = rrt.rtow(grid_half=grid_half, max_depth=8, image_width=32, samples_per_pixel=1)
            rng = np.random.default_rng(7)
            sets = []
            for _ in range(4):
                sp = sc.spheres.copy()
                sp["center_radius"][:, :3] += rng.normal(0.0, 0.05, (len(sp), 3)).astype(np.float32)
                sets.append(sp)
            ds = rrt.DeviceScene(sc, device=0, device_bvh=True)
            info = ds.bvh_info()
            line = {"tool": "scene_update_ab", "forms": True, "spheres": len(sc.spheres), "n_nodes": info["n_nodes"],
                    "max_depth": info["max_depth"]}
            try:
                for form in (0, 1):
                    _lib.refit_form(form)
                    try:
                        timed_refit(ds, sets[0], None)
                    except rrt.RrtError:
                        line[f"form{form}"] = None  # over the single workgroup's bound
                        continue
                    done = [timed_refit(ds, sets[(r + 1) % 4], None)[1] for r in range(max(args.rounds, 9))]
                    line[f"form{form}"] = stat(done)
                    line[f"form{form}_launches"] = ds.refit_stats()["last_launches"]
            finally:
                _lib.refit_form(-1)
            ds.close()
            print(json.dumps(line), flush=True)
        return 0

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
        fitted = rrt.DeviceScene(sc, device=0, device_bvh=True)
        timed_refit(fitted, sets[0], sc.motion)  # warm-up of (c): the first refit allocates
        line["first_refit"] = fitted.refit_stats()
        ms = {"recreate": [], "update": [], "refit_blocked": [], "refit": []}
        for r in range(args.rounds):
            k = (r + 1) % len(sets)
            t = time.perf_counter()
            again.close()
            again = rrt.DeviceScene(scenes[k], device=0, device_bvh=True)
            ms["recreate"].append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            kept.update_spheres(sets[k], sc.motion)
            ms["update"].append((time.perf_counter() - t) * 1e3)
            blocked, done = timed_refit(fitted, sets[k], sc.motion)
            ms["refit_blocked"].append(blocked)
            ms["refit"].append(done)
            print(f"{name} change round {r}: re-create {ms['recreate'][-1]:.3f} ms  update {ms['update'][-1]:.3f} ms  "
                  f"refit {done:.3f} ms (thread blocked {blocked:.3f} ms)", flush=True)
        line["steady_update"] = kept.update_stats()
        line["tree"] = {k: v for k, v in kept.bvh_info().items() if k in ("n_nodes", "max_depth", "node_stride")}
        line["recreate"] = stat(ms["recreate"])
        line["update"] = stat(ms["update"])
        line["update_median_below_recreate_min"] = statistics.median(ms["update"]) < min(ms["recreate"])
        line["speedup"] = round(statistics.median(ms["recreate"]) / statistics.median(ms["update"]), 2)
        line["steady_refit"] = fitted.refit_stats()
        line["refit"] = stat(ms["refit"])
        line["refit_blocked"] = stat(ms["refit_blocked"])
        line["refit_max_below_update_min"] = max(ms["refit"]) < min(ms["update"])
        line["refit_speedup"] = round(statistics.median(ms["update"]) / statistics.median(ms["refit"]), 2)
        again.close()

        # ---- quality: one frame over a refitted tree against a rebuilt one ----
        if args.quality:
            qtile = fitted.tile(16, 0, 1, 0, sc.spp)
            qbuf = torch.empty((sc.height, sc.width, 4), dtype=torch.float32, device="cuda:0")

            def frame_ms(ds):
                out = []
                for _ in range(5):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    ds.render_tile_async(qtile, qbuf.data_ptr(), stream.cuda_stream)
                    torch.cuda.synchronize()
                    out.append((time.perf_counter() - t) * 1e3)
                return min(out)

            line["quality"] = []
            for scale in (0.05, 0.4, 2.0):
                sp = sc.spheres.copy()
                sp["center_radius"][:, :3] += np.random.default_rng(12).normal(0.0, scale, (len(sp), 3)).astype(np.float32)
                fitted.update_spheres(sc.spheres, sc.motion)  # the build the refit starts from
                fitted.refit_spheres(sp, sc.motion, stream_ptr=stream.cuda_stream)
                cost = fitted.tree_cost()
                refit_ms = frame_ms(fitted)
                fitted.update_spheres(sp, sc.motion)
                rebuilt_ms = frame_ms(fitted)
                q = {"jitter": scale, "sah_ratio": round(cost["sah"] / cost["sah_at_build"], 4),
                     "frame_refit_ms": round(refit_ms, 3), "frame_rebuilt_ms": round(rebuilt_ms, 3),
                     "frame_ratio": round(refit_ms / rebuilt_ms, 4)}
                line["quality"].append(q)
                print(f"{name} quality: {q}", flush=True)

        # ---- the frame loop ----
        tile = kept.tile(16, 0, 1, 0, sc.spp)
        buf = torch.empty((sc.height, sc.width, 4), dtype=torch.float32, device="cuda:0")
        kept.render_tile_async(tile, buf.data_ptr(), stream.cuda_stream)  # warm-up frame
        torch.cuda.synchronize()
        loops = {"recreate": [], "update": [], "refit": [], "refit_or_rebuild": []}
        walk_rng = np.random.default_rng(77)  # the loop's sphere sets: a random walk away from the build
        walk = []
        sp = sc.spheres.copy()
        for _ in range(args.frames):
            sp = sp.copy()
            sp["center_radius"][:, :3] += walk_rng.normal(0.0, 0.05, (len(sp), 3)).astype(np.float32)
            walk.append(sp)
        rebuilds = 0
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
            t = time.perf_counter()
            for f in range(args.frames):
                fitted.refit_spheres(sets[f % len(sets)], sc.motion, stream_ptr=stream.cuda_stream)
                fitted.render_tile_async(tile, buf.data_ptr(), stream.cuda_stream)
            torch.cuda.synchronize()
            loops["refit"].append((time.perf_counter() - t) * 1e3)
            fitted.update_spheres(sc.spheres, sc.motion)
            torch.cuda.synchronize()
            rebuilds = 0
            t = time.perf_counter()
            for f in range(args.frames):
                fitted.refit_spheres(walk[f], sc.motion, stream_ptr=stream.cuda_stream)
                if f % args.cost_every == args.cost_every - 1:
                    cost = fitted.tree_cost()
                    if cost["sah"] > args.rebuild_at * cost["sah_at_build"]:
                        fitted.update_spheres(walk[f], sc.motion, stream_ptr=stream.cuda_stream)
                        rebuilds += 1
                fitted.render_tile_async(tile, buf.data_ptr(), stream.cuda_stream)
            torch.cuda.synchronize()
            loops["refit_or_rebuild"].append((time.perf_counter() - t) * 1e3)
            print(f"{name} {args.frames}-frame loop round {r}: re-create {loops['recreate'][-1]:.2f} ms  "
                  f"update {loops['update'][-1]:.2f} ms  refit {loops['refit'][-1]:.2f} ms  "
                  f"refit, rebuild past {args.rebuild_at} {loops['refit_or_rebuild'][-1]:.2f} ms ({rebuilds} rebuilds)", flush=True)
        kept.close()
        fitted.close()
        line["loop_frames"] = args.frames
        line["loop_recreate"] = stat(loops["recreate"])
        line["loop_update"] = stat(loops["update"])
        line["loop_refit"] = stat(loops["refit"])
        line["loop_refit_or_rebuild"] = dict(stat(loops["refit_or_rebuild"]), rebuild_at=args.rebuild_at, rebuilds=rebuilds)
        print(f"{name}: re-create {line['recreate']['median_ms']} ({line['recreate']['min_ms']}-{line['recreate']['max_ms']}) ms, "
              f"update {line['update']['median_ms']} ({line['update']['min_ms']}-{line['update']['max_ms']}) ms, "
              f"refit {line['refit']['median_ms']} ({line['refit']['min_ms']}-{line['refit']['max_ms']}) ms, "
              f"thread blocked {line['refit_blocked']['median_ms']} ms", flush=True)
        print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
