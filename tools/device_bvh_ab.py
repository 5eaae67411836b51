"""A/B of RRT_FLAG_DEVICE_BVH on one GPU: the same library with the flag off (the host sweep builder,
the default path) against the flag on (the binned builder on the device).

  creation   wall-clock of rrt_scene_create(_ex) + rrt_scene_destroy, flag off / on, in interleaved
             rounds after one warm-up each; every round is printed, then median and spread. The
             per-level read-back's share is estimated as levels x the round trip of one blocking 32-B
             device-to-host copy on an idle queue (measured here), levels = the kept tree's depth + 1
             (an LDS-shape build that was discarded adds its own levels: the share is a lower bound).
  render     the DeviceScene frame loop on each tree (device events over `--frames` frames), the rays
             per second from the scene's counters, and rrt_scene_count_work's node visits, box tests
             and primitive tests per ray.
  one-shot   wall-clock of rrt_hip_render (scene creation inside the call), flag off / on.

    python tools/device_bvh_ab.py [--scenes C2,NW1,NW9,C5,G160] [--rounds 7] [--width 480] [--spp 16]

G160 is the RTOW scene with grid_half = 160 (about 10^5 spheres). One JSON line per scene at the end.
"""
import argparse
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
    ap.add_argument("--scenes", default="C2,NW1,NW9,C5,G160")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--render", default="C2,NW9,C5", help="scenes whose render rate is measured on both trees")
    ap.add_argument("--one-shot", default="C5", help="scenes whose one-shot wall-clock is measured")
    args = ap.parse_args()

    import torch

    import rustraytrace_amd as rrt

    if not torch.cuda.is_available() or rrt.device_count() < 1:
        raise SystemExit("device_bvh_ab: no HIP device (this is a measurement: it does not run without one)")

    def scene_of(name):
        kw = dict(image_width=args.width, samples_per_pixel=args.spp)
        if name == "G160":
            sc = rrt.rtow(grid_half=160, max_depth=50, **kw)
        else:
            sc = rrt.named_scene(name, **kw)
        return sc

    # one blocking 32-B read on an idle queue: what each level of the device build waits for at least
    probe = torch.zeros(8, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    rt = []
    for _ in range(200):
        t = time.perf_counter()
        probe.cpu()
        rt.append((time.perf_counter() - t) * 1e3)
    read_ms = statistics.median(rt[20:])
    print(f"blocking 32-B device-to-host read: median {read_ms * 1e3:.1f} us", flush=True)

    for name in args.scenes.split(","):
        sc = scene_of(name)
        n_prims = len(sc.spheres) + (0 if sc.quads is None else len(sc.quads)) + (0 if sc.media is None else len(sc.media))
        line = {"tool": "device_bvh_ab", "scene": name, "primitives": n_prims, "image": [sc.width, sc.height],
                "spp": sc.spp}

        def create(flag):
            t = time.perf_counter()
            ds = rrt.DeviceScene(sc, device=0, device_bvh=flag)
            dt = (time.perf_counter() - t) * 1e3
            info = ds.bvh_info()
            ds.close()
            return dt, info

        ms, infos = {False: [], True: []}, {}
        for flag in (False, True):  # warm-up: code objects loaded, allocator primed
            _, infos[flag] = create(flag)
        first_off, _ = create(False)
        rounds = 2 if first_off > 2000.0 else args.rounds
        for r in range(rounds):
            for flag in (False, True):
                dt, _ = create(flag)
                ms[flag].append(dt)
            print(f"{name} creation round {r}: off {ms[False][-1]:.2f} ms  on {ms[True][-1]:.2f} ms", flush=True)
        levels = infos[True]["max_depth"] + 1
        line["creation_flag_off"] = stat(ms[False])
        line["creation_flag_on"] = stat(ms[True])
        line["creation_speedup"] = round(statistics.median(ms[False]) / statistics.median(ms[True]), 2)
        line["tree_flag_off"] = {k: infos[False][k] for k in ("n_nodes", "max_depth", "node_stride", "max_leaf_size")}
        line["tree_flag_on"] = {k: infos[True][k] for k in ("n_nodes", "max_depth", "node_stride", "max_leaf_size")}
        line["readback"] = {"levels_at_least": levels, "read_ms": round(read_ms, 4),
                            "share_of_creation_at_least": round(levels * read_ms / statistics.median(ms[True]), 3)}

        if name in args.render.split(","):
            stream = torch.cuda.current_stream()
            rates = {}
            for flag in (False, True):
                ds = rrt.DeviceScene(sc, device=0, device_bvh=flag)
                tile = ds.tile(16, 0, 1, 0, sc.spp)
                buf = torch.empty((sc.height, sc.width, 4), dtype=torch.float32, device="cuda:0")
                ds.render_tile_async(tile, buf.data_ptr(), stream.cuda_stream)  # warm-up frame
                torch.cuda.synchronize()
                ds.reset_counters()
                frame_ms = []
                for _ in range(args.frames):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    ds.render_tile_async(tile, buf.data_ptr(), stream.cuda_stream)
                    e1.record(stream)
                    torch.cuda.synchronize()
                    frame_ms.append(e0.elapsed_time(e1))
                rays = ds.counters()["rays"] / args.frames
                work = ds.count_work(tile)
                ds.close()
                rates["on" if flag else "off"] = {
                    "frame": stat(frame_ms), "grays_per_s": round(rays / statistics.median(frame_ms) / 1e6, 3),
                    "node_visits_per_ray": round(work["node_visits"] / work["rays"], 3),
                    "box_tests_per_ray": round(work["box_tests"] / work["rays"], 3),
                    "prim_tests_per_ray": round(work["sphere_tests"] / work["rays"], 3)}
                print(f"{name} render flag {'on' if flag else 'off'}: {rates['on' if flag else 'off']}", flush=True)
            line["render"] = rates

        if name in args.one_shot.split(","):
            shot = {False: [], True: []}
            for flag in (False, True):
                rrt.render(sc, device_bvh=flag)  # warm-up
            for r in range(args.rounds):
                for flag in (False, True):
                    t = time.perf_counter()
                    rrt.render(sc, device_bvh=flag)
                    shot[flag].append((time.perf_counter() - t) * 1e3)
                print(f"{name} one-shot round {r}: off {shot[False][-1]:.2f} ms  on {shot[True][-1]:.2f} ms", flush=True)
            line["one_shot_flag_off"] = stat(shot[False])
            line["one_shot_flag_on"] = stat(shot[True])
        print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
