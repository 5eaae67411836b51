"""A/B of the two device builders behind rrt_scene_update_* on one GPU: the binned SAH builder
(RRT_FLAG_DEVICE_BVH) against the LBVH (RRT_FLAG_FAST_BVH), in scene_update_ab.py's protocol.

  change     wall-clock of one update of the spheres, in interleaved rounds after one warm-up each (the
             scene's first update, which allocates); every round is printed, then median (min-max).
             Arms: the binned update of this library; the LBVH update of this library; and, with
             `--parent-lib`, the binned update of another build of the library (the parent commit's),
             which a child process runs (RRT_LIB_PATH) in the same rounds: it must not have moved.
             NW9 (final_scene) is updated through rrt_scene_update_world, the others through
             rrt_scene_update_spheres.
  loop       `--frames` frames at `--width` x `--spp` that update the spheres before every frame and
             render it on one stream, timed as a whole, with either builder.
  trace      at `--trace-width` x `--trace-spp`: one frame's time over either tree (min of 3), its rays,
             and rrt_scene_count_work's node visits, box tests and primitive tests per ray.

    python tools/fast_bvh_ab.py [--scenes C2,NW1,C5,G160,NW9] [--rounds 7] [--width 480] [--spp 16] [--frames 16]
                                [--trace-width 1920] [--trace-spp 32] [--parent-lib PATH]

G160 is the RTOW scene with grid_half = 160 (about 10^5 spheres). The sphere sets are seeded jitters of
the scene's centers. One JSON line per scene at the end.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stat(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "n": len(v)}


def scene_of(rrt, name, width, spp):
    kw = dict(image_width=width, samples_per_pixel=spp)
    if name == "G160":
        return rrt.rtow(grid_half=160, max_depth=50, **kw)
    return rrt.named_scene(name, **kw)


def sphere_sets(np, sc):
    rng = np.random.default_rng(2024)
    sets = []
    for _ in range(8):
        sp = sc.spheres.copy()
        sp["center_radius"][:, :3] += rng.normal(0.0, 0.05, (len(sp), 3)).astype(np.float32)
        sets.append(sp)
    return sets


def update(ds, name, spheres, motion, stream_ptr=0):
    if name == "NW9":
        ds.update_world(spheres=spheres, motion=motion, stream_ptr=stream_ptr)
    else:
        ds.update_spheres(spheres, motion, stream_ptr=stream_ptr)


def child(args):
    """The other library's binned arm: one update per line "u K" on stdin, its milliseconds on stdout."""
    import numpy as np

    import rustraytrace_amd as rrt

    name = args.child
    sc = scene_of(rrt, name, args.width, args.spp)
    sets = sphere_sets(np, sc)
    ds = rrt.DeviceScene(sc, device=0, device_bvh=True)
    update(ds, name, sets[0], sc.motion)
    print("ready", flush=True)
    for line in sys.stdin:
        if not line.startswith("u "):
            break
        k = int(line.split()[1])
        t = time.perf_counter()
        update(ds, name, sets[k], sc.motion)
        print(f"{(time.perf_counter() - t) * 1e3:.6f}", flush=True)
    ds.close()
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scenes", default="C2,NW1,C5,G160,NW9")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--trace-width", type=int, default=1920)
    ap.add_argument("--trace-spp", type=int, default=32)
    ap.add_argument("--parent-lib", default=None, help="another build of librrt_hip.so for the third arm")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)

    import numpy as np
    import torch

    import rustraytrace_amd as rrt

    if not torch.cuda.is_available() or rrt.device_count() < 1:
        raise SystemExit("fast_bvh_ab: no HIP device (this is a measurement: it does not run without one)")
    stream = torch.cuda.current_stream()

    for name in args.scenes.split(","):
        sc = scene_of(rrt, name, args.width, args.spp)
        sets = sphere_sets(np, sc)
        line = {"tool": "fast_bvh_ab", "scene": name, "spheres": len(sc.spheres), "image": [sc.width, sc.height], "spp": sc.spp}
        other = None
        if args.parent_lib:
            env = dict(os.environ, RRT_LIB_PATH=os.path.abspath(args.parent_lib))
            other = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", name, "--width", str(args.width),
                                      "--spp", str(args.spp)], env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
            if other.stdout.readline().strip() != "ready":
                raise SystemExit("fast_bvh_ab: the parent library's arm did not start")

        # ---- one change ----
        arms = {"binned": rrt.DeviceScene(sc, device=0, device_bvh=True), "lbvh": rrt.DeviceScene(sc, device=0, fast_bvh=True)}
        for ds in arms.values():
            update(ds, name, sets[0], sc.motion)  # warm-up: the first update allocates
        ms = {"binned_parent": [], "binned": [], "lbvh": []}
        for r in range(args.rounds):
            k = (r + 1) % len(sets)
            if other:
                other.stdin.write(f"u {k}\n")
                other.stdin.flush()
                ms["binned_parent"].append(float(other.stdout.readline()))
            for arm, ds in arms.items():
                t = time.perf_counter()
                update(ds, name, sets[k], sc.motion)
                ms[arm].append((time.perf_counter() - t) * 1e3)
            print(f"{name} change round {r}: " + "  ".join(f"{a} {v[-1]:.3f} ms" for a, v in ms.items() if v), flush=True)
        if other:
            other.stdin.write("q\n")
            other.stdin.flush()
            other.wait(timeout=60)
        for arm, ds in arms.items():
            line[f"update_{arm}"] = stat(ms[arm])
            line[f"stats_{arm}"] = dict(ds.build_stats(), allocations=ds.update_stats()["last_allocations"])
            line[f"tree_{arm}"] = {k: v for k, v in ds.bvh_info().items() if k in ("n_nodes", "max_depth", "node_stride")}
        if other:
            line["update_binned_parent"] = stat(ms["binned_parent"])
        line["lbvh_max_below_binned_min"] = max(ms["lbvh"]) < min(ms["binned"])
        line["speedup"] = round(statistics.median(ms["binned"]) / statistics.median(ms["lbvh"]), 2)

        # ---- the frame loop ----
        tile = arms["binned"].tile(16, 0, 1, 0, sc.spp)
        buf = torch.empty((sc.height, sc.width, 4), dtype=torch.float32, device="cuda:0")
        loops = {"binned": [], "lbvh": []}
        for arm, ds in arms.items():
            ds.render_tile_async(tile, buf.data_ptr(), stream.cuda_stream)  # warm-up frame
        torch.cuda.synchronize()
        for r in range(3):
            for arm, ds in arms.items():
                t = time.perf_counter()
                for f in range(args.frames):
                    update(ds, name, sets[f % len(sets)], sc.motion, stream_ptr=stream.cuda_stream)
                    ds.render_tile_async(tile, buf.data_ptr(), stream.cuda_stream)
                torch.cuda.synchronize()
                loops[arm].append((time.perf_counter() - t) * 1e3)
            print(f"{name} {args.frames}-frame loop round {r}: " + "  ".join(f"{a} {v[-1]:.2f} ms" for a, v in loops.items()), flush=True)
        line["loop_frames"] = args.frames
        for arm, ds in arms.items():
            line[f"loop_{arm}"] = stat(loops[arm])
            ds.close()

        # ---- tracing either tree ----
        big = scene_of(rrt, name, args.trace_width, args.trace_spp)
        for arm, kw in (("binned", dict(device_bvh=True)), ("lbvh", dict(fast_bvh=True))):
            ds = rrt.DeviceScene(big, device=0, **kw)
            ttile = ds.tile(16, 0, 1, 0, big.spp)
            tbuf = torch.empty((big.height, big.width, 4), dtype=torch.float32, device="cuda:0")
            times = []
            for _ in range(4):  # the first is the warm-up
                ds.reset_counters()
                torch.cuda.synchronize()
                t = time.perf_counter()
                ds.render_tile_async(ttile, tbuf.data_ptr(), stream.cuda_stream)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t) * 1e3)
            rays = int(ds.counters()["rays"])
            work = ds.count_work(ttile)
            ds.close()
            best = min(times[1:])
            per_ray = {k: round(int(v) / max(int(work.get("rays", rays)), 1), 3) for k, v in work.items() if k != "rays"}
            line[f"trace_{arm}"] = {"frame_ms": round(best, 3), "rays": rays, "mrays_per_s": round(rays / best / 1e3, 1),
                                    "work_per_ray": per_ray}
            del tbuf
        line["trace_rate_lbvh_over_binned"] = round(line["trace_lbvh"]["mrays_per_s"] / line["trace_binned"]["mrays_per_s"], 4)
        u = {a: line[f"update_{a}"] for a in ("binned", "lbvh")}
        print(f"{name}: update binned {u['binned']['median_ms']} ({u['binned']['min_ms']}-{u['binned']['max_ms']}) ms, "
              f"lbvh {u['lbvh']['median_ms']} ({u['lbvh']['min_ms']}-{u['lbvh']['max_ms']}) ms; trace rate lbvh / binned "
              f"{line['trace_rate_lbvh_over_binned']}", flush=True)
        print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
