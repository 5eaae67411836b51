"""A/B of the books path's output step on one GPU: the wall-clock of a frame from the call to the
written P6, by the route through the host quantiser against the device one.

  host route    rrt_hip_render_f64 (32 B/pixel of f64 sums to the host), rrt_quantize_accum_books_f64
                on the host, rrt_write_pnm_from_rgb8 (P6)
  device route  rrt_hip_render_f64_rgb8 (color.rs on the device, 3 B/pixel to the host), the same write

Both routes run in this one process, after one warm-up call each, in interleaved rounds (host,
device, host, ...); every round's wall-clock is printed, then the medians and the spread (min, max)
per route. The two P6 files must be byte-equal. The quantiser kernel's own time is then taken with
device events over `--reps` back-to-back launches on the frame's f64 sums, next to the event time of
the frame's render (rrt_render_tile_f64_async). One JSON line at the end.

    python tools/books_output_ab.py [--config C2] [--width W] [--spp S] [--rounds 8] [--out-dir DIR]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", default="C2")
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--spp", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20, help="quantiser launches per event-timed window")
    ap.add_argument("--out-dir", default=None, help="where the P6 files go (default: a temporary directory)")
    args = ap.parse_args()

    import torch

    import rustraytrace_amd as rrt

    if not torch.cuda.is_available() or rrt.device_count() < 1:
        raise SystemExit("books_output_ab: no HIP device (this is a measurement: it does not run without one)")
    over = {k: v for k, v in (("image_width", args.width), ("samples_per_pixel", args.spp)) if v}
    scene = rrt.config_scene(args.config, **over)
    W, H, S = scene.width, scene.height, scene.spp
    out_dir = args.out_dir or tempfile.mkdtemp(prefix="books_output_ab_")
    os.makedirs(out_dir, exist_ok=True)
    paths = {"host": os.path.join(out_dir, "host.ppm"), "device": os.path.join(out_dir, "device.ppm")}

    def host_route():
        sums = rrt.render_f64(scene)
        rgb8 = rrt.quantize_accum_books_f64(W, H, sums, S)
        rrt.write_pnm_from_rgb8(W, H, rgb8, True, paths["host"])

    def device_route():
        rgb8 = rrt.render_f64_rgb8(scene)
        rrt.write_pnm_from_rgb8(W, H, rgb8, True, paths["device"])

    routes = {"host": host_route, "device": device_route}
    for fn in routes.values():  # warm-up: code objects loaded, allocations made once
        fn()
    with open(paths["host"], "rb") as a, open(paths["device"], "rb") as b:
        equal = a.read() == b.read()
    print(f"{args.config} {W}x{H}x{S}: P6 files byte-equal: {equal}", flush=True)
    ms = {k: [] for k in routes}
    for r in range(args.rounds):
        for name, fn in routes.items():
            t = time.perf_counter()
            fn()  # ends in the file write, after the library's own device synchronise
            ms[name].append((time.perf_counter() - t) * 1e3)
        print(f"round {r}: host {ms['host'][-1]:.2f} ms  device {ms['device'][-1]:.2f} ms", flush=True)

    # the kernels' own times (device events): the frame's render, then the quantiser over its sums
    ds = rrt.DeviceScene(scene, device=0, f64=True)
    tile = ds.tile(16, 0, 1, 0, S)
    sums = torch.empty((H, W, 4), dtype=torch.float64, device="cuda:0")
    rgb8 = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.current_stream()
    render_ms, quant_ms = [], []
    for i in range(4):  # the first pass is the warm-up
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record(stream)
        ds.render_tile_f64_async(tile, sums.data_ptr(), stream.cuda_stream)
        e1.record(stream)
        for _ in range(args.reps):
            rrt.quantize_accum_books_async(W * H, sums.data_ptr(), S, rgb8.data_ptr(), stream.cuda_stream, f64=True)
        e2.record(stream)
        torch.cuda.synchronize()
        if i:
            render_ms.append(e0.elapsed_time(e1))
            quant_ms.append(e1.elapsed_time(e2) / args.reps)
    ds.close()
    same = bool((rgb8.cpu().numpy() == rrt.quantize_accum_books_f64(W, H, sums.cpu().numpy(), S)).all())

    def stat(v):
        return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}

    line = {
        "tool": "books_output_ab", "config": args.config, "image": [W, H], "spp": S, "rounds": args.rounds,
        "p6_equal": equal, "host_route": stat(ms["host"]), "device_route": stat(ms["device"]),
        "saving_ms": round(statistics.median(ms["host"]) - statistics.median(ms["device"]), 3),
        "d2h_bytes": {"host_route": W * H * 32, "device_route": W * H * 3},
        "render_kernel_ms_events": stat(render_ms),
        "quantiser_kernel_ms_events": {**stat(quant_ms), "launches_per_window": args.reps, "bytes_equal_host": same},
    }
    print(json.dumps(line), flush=True)
    return 0 if equal and same else 1


if __name__ == "__main__":
    sys.exit(main())
