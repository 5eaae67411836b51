"""Wall time of the three ways to change a scene's quads on one GPU:

  (a) re-create   rrt_scene_destroy + rrt_scene_create_ex with RRT_FLAG_DEVICE_BVH of the new inputs,
                  the only way before rrt_scene_update_geometry existed (`--arm recreate`; run it on
                  the parent's library with RRT_LIB_PATH to time the parent itself);
  (b) update      rrt_scene_update_geometry on the scene that is kept: a rebuild on the device;
  (c) refit       rrt_scene_refit_geometry on a scene that is kept, as the enqueue-to-event time (two
                  events on the stream around the call, read after a synchronisation) beside the wall
                  time the call blocks the calling thread.

Scenes: `cornell` (the_next_week 7: 18 quads) and `quads300` (300 random quads and 40 spheres). The
quad sets are seeded jitters of the scene's quads. One warm-up per arm (the first update and the first
refit allocate), then `--rounds` rounds, every round printed, then median (min-max) and one JSON line
per scene. All arms go through the Python wrappers, whose own cost is part of every wall-time figure.

    python tools/scene_geometry_ab.py [--arm all|recreate] [--scenes cornell,quads300] [--rounds 9]
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
    ap.add_argument("--scenes", default="cornell,quads300")
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()

    import numpy as np
    import torch

    import rustraytrace_amd as rrt
    from rustraytrace_amd import _lib
    from rustraytrace_amd import scenes as S

    if not torch.cuda.is_available() or rrt.device_count() < 1:
        raise SystemExit("scene_geometry_ab: no HIP device (this is a measurement: it does not run without one)")

    def quads300():
        rng = np.random.default_rng(7)
        mats = np.concatenate([S._material(0, (0.6, 0.3, 0.2)), S._material(1, (0.8, 0.8, 0.9), fuzz=0.1),
                               S._material(2, (1.0, 1.0, 1.0), ref_idx=1.5), S._material(4, (3.0, 3.0, 2.5))])
        sph = np.concatenate([S._sphere(tuple(rng.uniform(-20, 20, 3)), rng.uniform(0.5, 2.0), k % len(mats))
                              for k in range(40)])
        quads = np.zeros(300, dtype=_lib.QUAD_DTYPE)
        quads["q"][:, :3] = rng.uniform(-20, 20, (300, 3))
        quads["u"][:, :3] = rng.normal(0, 2, (300, 3))
        quads["v"][:, :3] = rng.normal(0, 2, (300, 3))
        quads["material_index"] = np.arange(300) % len(mats)
        cam = S.make_camera(aspect_ratio=16.0 / 9.0, image_width=32, samples_per_pixel=4, max_depth=8, vfov=50.0,
                            lookfrom=(0.0, 5.0, 45.0), lookat=(0.0, 0.0, 0.0), n_spheres=len(sph))
        return S.SceneData(cam, sph, mats, flags=_lib.FLAG_RAY_TIME, name="quads300", quads=quads)

    def scene_of(name):
        if name == "cornell":
            return rrt.next_week_scene(7, dict(image_width=32, samples_per_pixel=4))
        if name == "quads300":
            return quads300()
        raise SystemExit(f"scene_geometry_ab: unknown scene {name!r}")

    stream = torch.cuda.current_stream()
    for name in args.scenes.split(","):
        sc = scene_of(name)
        rng = np.random.default_rng(2024)
        sets = []
        for _ in range(8):
            q = sc.quads.copy()
            ext = np.maximum(np.linalg.norm(q["u"][:, :3], axis=1), np.linalg.norm(q["v"][:, :3], axis=1))[:, None]
            for k in ("q", "u", "v"):
                q[k][:, :3] += (rng.normal(0.0, 0.01, (len(q), 3)) * ext).astype(np.float32)
            sets.append(q)
        scenes = [dataclasses.replace(sc, quads=q) for q in sets]
        line = {"tool": "scene_geometry_ab", "arm": args.arm, "scene": name, "quads": len(sc.quads), "spheres": len(sc.spheres),
                "library": os.environ.get("RRT_LIB_PATH", "this build")}
        ms = {"recreate": [], "update": [], "refit_event": [], "refit_blocked": []}
        again = rrt.DeviceScene(sc, device=0, device_bvh=True)  # warm-up of (a)
        if args.arm == "all":
            kept = rrt.DeviceScene(sc, device=0, device_bvh=True)
            kept.update_geometry(quads=sets[0])  # warm-up of (b)
            fitted = rrt.DeviceScene(sc, device=0, device_bvh=True)
            fitted.refit_geometry(quads=sets[0], stream_ptr=stream.cuda_stream)  # warm-up of (c)
            torch.cuda.synchronize()
        for r in range(args.rounds):
            k = (r + 1) % len(sets)
            torch.cuda.synchronize()
            t = time.perf_counter()
            again.close()
            again = rrt.DeviceScene(scenes[k], device=0, device_bvh=True)
            ms["recreate"].append((time.perf_counter() - t) * 1e3)
            if args.arm == "all":
                t = time.perf_counter()
                kept.update_geometry(quads=sets[k])
                ms["update"].append((time.perf_counter() - t) * 1e3)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                t = time.perf_counter()
                fitted.refit_geometry(quads=sets[k], stream_ptr=stream.cuda_stream)
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
            line["tree"] = {k2: v for k2, v in kept.bvh_info().items() if k2 in ("n_nodes", "max_depth", "node_stride")}
            line["refit_launches"] = fitted.refit_stats()["last_launches"]
            kept.close()
            fitted.close()
        print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
