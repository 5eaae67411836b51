"""Mrays/s of the ray queries (rrt_scene_primary_hits_async, rrt_scene_query_async) on C2, C5 and
cornell_box at 1920x1080, one GPU: HIP-event time over `--iters` launches after a warm-up, for the
primary-hit launch (rays formed in the kernel, 8x8 tiles) and for the same rays passed as an array
(row-major order), in both modes; beside them the render's Grays/s from the same run, for context (a
render ray is a bounce of a path: incoherent, and shaded). The surface leg times the same two launches
with RrtSurface records (rrt_scene_primary_surface_async, rrt_scene_surface_async: 64 B written per ray
against 8), on those scenes and on final_scene, whose media only the surface entries accept.
One JSON object per line; a table on stderr. --repeats N times every query leg N times and reports the
median and the spread (max - min) / median: the run-to-run margin an A/B of two builds is read against.

    python tools/bench_query.py [--iters 20] > profiles/query_scenes.jsonl
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def scenes(spp_scale):
    import rustraytrace_amd as rrt

    def s(n):
        return max(1, int(n * spp_scale))

    yield "C2 rtow 1920x1080", rrt.config_scene("C2", samples_per_pixel=s(512))
    yield "C5 rtow 10k spheres 1920x1080", rrt.config_scene("C5", samples_per_pixel=s(256))
    yield "NW7 cornell_box 1920x1080", rrt.next_week_scene(7, dict(aspect_ratio=16.0 / 9.0, image_width=1920, max_depth=50,
                                                                   samples_per_pixel=s(256)))
    # constant media: the surface leg only
    yield "NW9 final_scene 1920x1080", rrt.next_week_scene(9, dict(aspect_ratio=16.0 / 9.0, image_width=1920, max_depth=40,
                                                                   samples_per_pixel=s(64)))


def camera_rays(cam):
    """The primary-hit entry's rays in row-major order (tests/test_gpu_ray_query.py camera_rays)."""
    import numpy as np

    from rustraytrace_amd import _lib

    c = cam[0]
    w, h = int(c["params_f"][1]), int(c["params_f"][2])
    org, p00, du, dv = (np.asarray(c[k][:3], dtype=np.float32) for k in ("origin", "pixel00", "pixel_delta_u", "pixel_delta_v"))
    x = np.arange(w, dtype=np.float32)[None, :, None]
    y = np.arange(h, dtype=np.float32)[:, None, None]
    d = ((p00 + du * x) + dv * y) - org
    r = np.zeros(h * w, dtype=_lib.RAY_DTYPE)
    r["o"], r["d"], r["tmax"] = org, d.reshape(-1, 3), np.inf
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--spp-scale", type=float, default=0.125, help="of the render leg's samples per pixel")
    ap.add_argument("--repeats", type=int, default=1, help="timings per query leg: the median, and their spread")
    ap.add_argument("--no-render", action="store_true", help="skip the render leg")
    ap.add_argument("--no-surface", action="store_true", help="skip the surface leg (a build without the entries)")
    a = ap.parse_args()
    assert a.iters >= 20, "at least 20 launches per figure"
    import numpy as np
    import torch

    import rustraytrace_amd as rrt
    from rustraytrace_amd import _lib

    stream = torch.cuda.current_stream()

    def timed_once(launch, iters):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        for _ in range(iters):
            launch()
        t1.record(stream)
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / iters

    spreads = {}

    def timed(launch, iters, key=None):
        launch()  # warm-up (the first query also allocates the order table)
        torch.cuda.synchronize()
        ms = sorted(timed_once(launch, iters) for _ in range(max(1, a.repeats)))
        med = ms[len(ms) // 2]
        if key is not None:
            spreads[key] = round((ms[-1] - ms[0]) / med, 4)
        return med

    rows = []
    for name, sc in scenes(a.spp_scale):
        if a.no_surface and sc.media is not None and len(sc.media) > 0:
            continue  # only the surface entries accept constant media: no leg to time
        ds = rrt.DeviceScene(sc)
        n = sc.width * sc.height
        rays = camera_rays(sc.camera)
        d_rays = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).to("cuda:0")
        d_hits = torch.zeros(n * 2, dtype=torch.int32, device="cuda:0")
        d_hits2 = torch.zeros(n * 2, dtype=torch.int32, device="cuda:0")
        row = dict(scene=name, width=sc.width, height=sc.height, rays=n, iters=a.iters, repeats=a.repeats,
                   bvh_nodes=ds.bvh_info()["n_nodes"], node_stride=ds.bvh_info()["node_stride"])
        spreads.clear()
        media = sc.media is not None and len(sc.media) > 0
        row["array_equals_primary"] = True
        if not media:  # the plain queries refuse constant media
            ms = timed(lambda: ds.primary_hits_async(d_hits.data_ptr(), 0.0, stream.cuda_stream), a.iters, "primary")
            row["primary_ms"], row["primary_mrays_per_s"] = round(ms, 4), round(n / ms / 1e3, 1)
            for mode in ("closest", "any"):
                ms = timed(lambda: ds.query_async(d_rays.data_ptr(), n, d_hits2.data_ptr(), mode, stream.cuda_stream), a.iters,
                           f"array_{mode}")
                row[f"array_{mode}_ms"], row[f"array_{mode}_mrays_per_s"] = round(ms, 4), round(n / ms / 1e3, 1)
            ds.query_async(d_rays.data_ptr(), n, d_hits2.data_ptr(), "closest", stream.cuda_stream)
            torch.cuda.synchronize()
            row["array_equals_primary"] = bool((d_hits == d_hits2).all().item())
            row["hit_fraction"] = round(float((d_hits.view(-1, 2)[:, 1] != -1).float().mean().item()), 4)
        if not a.no_surface:  # the surface leg: the same two launches with 64-B records
            d_surf = torch.zeros(n * 16, dtype=torch.int32, device="cuda:0")
            d_surf2 = torch.zeros(n * 16, dtype=torch.int32, device="cuda:0")
            ms = timed(lambda: ds.primary_surface_async(d_surf.data_ptr(), 0.0, stream.cuda_stream), a.iters, "surface_primary")
            row["surface_primary_ms"], row["surface_primary_mrays_per_s"] = round(ms, 4), round(n / ms / 1e3, 1)
            ms = timed(lambda: ds.surface_async(d_rays.data_ptr(), n, d_surf2.data_ptr(), stream.cuda_stream), a.iters, "surface_array")
            row["surface_array_ms"], row["surface_array_mrays_per_s"] = round(ms, 4), round(n / ms / 1e3, 1)
            torch.cuda.synchronize()
            same = bool((d_surf == d_surf2).all().item())
            if not media:  # (prim, t) of the records are the closest query's
                rec = d_surf.view(-1, 16)
                same = same and bool((rec[:, 3] == d_hits.view(-1, 2)[:, 0]).all().item() and (rec[:, 7] == d_hits.view(-1, 2)[:, 1]).all().item())
                row["surface_over_closest"] = round(row["surface_array_ms"] / row["array_closest_ms"], 3)
            else:
                row["hit_fraction"] = round(float((d_surf.view(-1, 16)[:, 7] != -1).float().mean().item()), 4)
            row["array_equals_primary"] = row["array_equals_primary"] and same
            del d_surf, d_surf2
        row["spread"] = dict(spreads)
        if a.no_render:
            ds.close()
            rows.append(row)
            print(json.dumps(row), flush=True)
            continue
        # the render of the same scene in the same run
        tile = ds.tile(16, 0, 1, 0, sc.spp)
        buf = torch.empty((sc.height, sc.width, 4), dtype=torch.float32, device="cuda:0")
        ds.render_tile_async(tile, buf.data_ptr(), stream.cuda_stream)
        torch.cuda.synchronize()
        ds.reset_counters()
        r_iters = 3
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        for _ in range(r_iters):
            ds.render_tile_async(tile, buf.data_ptr(), stream.cuda_stream)
        t1.record(stream)
        torch.cuda.synchronize()
        r_ms = t0.elapsed_time(t1) / r_iters
        r_rays = ds.counters()["rays"] / r_iters
        row["render_spp"], row["render_ms"], row["render_grays_per_s"] = sc.spp, round(r_ms, 3), round(r_rays / r_ms / 1e6, 2)
        ds.close()
        rows.append(row)
        print(json.dumps(row), flush=True)
    print(f"{'scene':32s} {'primary':>9s} {'array':>9s} {'any':>9s} {'surf prim':>9s} {'surf arr':>9s}  Mrays/s | render Grays/s",
          file=sys.stderr)
    for r in rows:
        print(f"{r['scene']:32s} {r.get('primary_mrays_per_s', 0):9.0f} {r.get('array_closest_mrays_per_s', 0):9.0f} "
              f"{r.get('array_any_mrays_per_s', 0):9.0f} {r.get('surface_primary_mrays_per_s', 0):9.0f} "
              f"{r.get('surface_array_mrays_per_s', 0):9.0f}          | {r.get('render_grays_per_s', 0):.2f}", file=sys.stderr)
    return 0 if all(r["array_equals_primary"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
