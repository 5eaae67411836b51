"""A/B of multi_gpu's gather on the f64 books path: `--f64` (f64 accum tiles, 32 B/pixel, quantised on
rank 0) against `--f64 --gather rgb8` (each rank quantises on the device, 3 B/pixel gathered), as
launches of rustraytrace_amd.multi_gpu under torch.distributed.run, alternating, each under a time
limit; the first failure ends the run. With `--backend gloo` the ranks share one GPU: a rehearsal
of the data path (host copies gathered over loopback), not a scaling result. Prints each launch's
JSON line, then the medians and spread of gather_ms per mode and whether the PPMs are byte-equal.

    python tools/books_gather_ab.py [--ranks 2] [--config C2] [--width W] [--spp S] [--rounds 4] [--backend gloo]
"""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--config", default="C2")
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--spp", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--backend", default="gloo")
    ap.add_argument("--timeout", type=int, default=150, help="seconds per launch")
    args = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="books_gather_ab_")
    common = ["--config", args.config, "--backend", args.backend, "--f64", "--p6"]
    if args.width:
        common += ["--width", str(args.width)]
    if args.spp:
        common += ["--spp", str(args.spp)]
    modes = {"accum": [], "rgb8": ["--gather", "rgb8"]}
    lines = {k: [] for k in modes}
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), OMP_NUM_THREADS="1")
    for r in range(args.rounds + 1):  # round 0 is the warm-up (file caches, first use of the box)
        for name, extra in modes.items():
            out = os.path.join(tmp, name + ".ppm")
            cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.ranks}",
                   "--master-addr", "127.0.0.1", f"--master-port={free_port()}", "-m", "rustraytrace_amd.multi_gpu"]
            p = subprocess.run(cmd + common + extra + ["--out", out], capture_output=True, text=True, cwd=ROOT,
                               env=env, timeout=args.timeout)
            if p.returncode != 0:
                print(p.stderr[-2000:], file=sys.stderr)
                return 1
            line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            print(("warm-up " if r == 0 else f"round {r} ") + name + ": " + json.dumps(line), flush=True)
            if r:
                lines[name].append(line)
    with open(os.path.join(tmp, "accum.ppm"), "rb") as a, open(os.path.join(tmp, "rgb8.ppm"), "rb") as b:
        equal = a.read() == b.read()

    def stat(v):
        return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}

    first = lines["accum"][0]
    px = first["image"][0] * first["image"][1]
    print(json.dumps({
        "tool": "books_gather_ab", "config": args.config, "image": first["image"], "spp": first["spp"],
        "ranks": args.ranks, "backend": args.backend, "rounds": args.rounds, "ppm_equal": equal,
        "note": "ranks share one GPU over gloo: a rehearsal, not a scaling result" if args.backend == "gloo" else None,
        "gather_ms": {k: stat([ln["gather_ms"] for ln in v]) for k, v in lines.items()},
        "gather_bytes": {"accum": px * 32, "rgb8": px * 3},
        "kernel_ms_max_over_ranks": {k: stat([ln["kernel_ms_max_over_ranks"] for ln in v]) for k, v in lines.items()},
    }), flush=True)
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
