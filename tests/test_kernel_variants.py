"""Every compile-time arm left in the kernel sources is the shipped default or compiled here.

The sources keep only debug builds (-DRRT_PHASE_TIMING=1..9 and -DRRT_F64_STATS=1..5: per-wave
statistics, -DRRT_TRACE_X/Y/S: a printf trace of one path, the RRT_DEBUG_* pricing builds), numeric
tuning knobs (launch shapes, issue priorities, the work-unit tile, chunk sizes) and the two f64 arms
that have tests of their own (RRT_F64_SPHERE32, RRT_F64_REJ32). Rejected variants are deleted
(DESIGN.md §4 / §5 keep their measurements). Each non-default arm is type-checked for gfx950 here (hipcc -fsyntax-only
instantiates every kernel template the launch functions reference), so none of them rots.
CPU only: hipcc cross-compiles without a GPU.
"""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rustraytrace_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

# Independent switches share an entry (a variant compiles every .hip file once, and most switches
# touch one of the two), so a new switch rarely costs a compile of its own.
VARIANTS = {
    # per-wave statistics of both kernels (RRT_F64_STATS has modes 1-5)
    "phase1": ["-DRRT_PHASE_TIMING=1", "-DRRT_F64_STATS=1"],
    "phase2": ["-DRRT_PHASE_TIMING=2", "-DRRT_F64_STATS=2"],
    "phase3": ["-DRRT_PHASE_TIMING=3", "-DRRT_F64_STATS=3"],
    "phase4": ["-DRRT_PHASE_TIMING=4", "-DRRT_F64_STATS=4"],
    "phase5": ["-DRRT_PHASE_TIMING=5", "-DRRT_F64_STATS=5"],
    # and the debug builds that price node bytes (1) and one more L2 round trip per node (2)
    "phase6": ["-DRRT_PHASE_TIMING=6", "-DRRT_DEBUG_EXTRA_NODE_LOAD=1"],
    "phase7": ["-DRRT_PHASE_TIMING=7", "-DRRT_DEBUG_EXTRA_NODE_LOAD=2"],
    "phase8": ["-DRRT_PHASE_TIMING=8"],
    "phase9": ["-DRRT_PHASE_TIMING=9"],
    # the debug stand-ins that price the noise texture, the texel angles (f32, f64) and the
    # rejection loops (wrong images)
    "noise": ["-DRRT_DEBUG_NOISE_FIXED=1", "-DRRT_DEBUG_TEXEL_FIXED=1", "-DRRT_DEBUG_F64_TEXEL_FIXED=1",
              "-DRRT_DEBUG_NOREJECT=1"],
    "trace": ["-DRRT_TRACE_X=3", "-DRRT_TRACE_Y=4", "-DRRT_TRACE_S=5"],
    # round-6 launch shapes back at their earlier values; the media class's own wave count
    "launch_knobs": ["-DRRT_B1U_WAVES=6", "-DRRT_B1U_BLOCK=512", "-DRRT_B1D_WAVES=6", "-DRRT_B3_WAVES=1",
                     "-DRRT_B2_NF_WAVES=5", "-DRRT_B1_GLOBAL_WAVES=6", "-DRRT_B2_MEDIA_GLOBAL_WAVES=4"],
    # (RRT_F16_ORDERED_MAX_CLASS=0: the ordered f16 slab for book 1 only)
    "knobs": ["-DRRT_BLOCK=256", "-DRRT_WAVES=4", "-DRRT_TILE_W=16", "-DRRT_B2_WAVES=1", "-DRRT_B2_BLOCK=512",
              "-DRRT_PRIO_REFILL=0", "-DRRT_PRIO_NODE=0", "-DRRT_PRIO_LEAF=0", "-DRRT_PRIO_SHADE=0",
              "-DRRT_F16_ORDERED_MAX_CLASS=0"],
    # rrt_books64.hip: launch shape, LDS budget and fold group; the f32 sphere pre-test
    # (tests/test_sphere32_conservative.py) and the f32 rejection test (tests/test_rejection_exact.py)
    "f64_knobs": ["-DRRT_F64_BLOCK=256", "-DRRT_F64_WAVES=2", "-DRRT_F64_LDS512_KB=32", "-DRRT_F64_FOLD_GROUP=2",
                  "-DRRT_F64_SPHERE32=1", "-DRRT_F64_REJ32=1"],
}
# rrt_host.cpp's numbers (chunk and tail-unit sizes, history lanes) and the forced chunk of A/B builds
HOST_VARIANT = ["-DRRT_TAIL_DIV=8", "-DRRT_TAIL_DIV_LO=4", "-DRRT_F64_TAIL_DIV=2", "-DRRT_F64_TAIL_DIV_HI=4",
                "-DRRT_F64_TS_DIV=4", "-DRRT_F64_HIST_LANES_PER_CU=512", "-DRRT_CHUNK_FORCE=32"]
# switches with a test of their own: the host/device macro and the reciprocal form of the
# conservative f32 tests' harnesses (tests/box32, tests/sphere32), tests/test_rng_bitop3.py
TESTED_ELSEWHERE = {"RRT_HD", "RRT_BOX32_RCP", "RRT_RNG_BITOP3"}


def type_check(src, flags):
    cmd = [HIPCC, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-Wall", "-Wno-unused-function",
           "-Wno-unused-command-line-argument", *flags, os.path.join(CSRC, src)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"{src} {flags}:\n{r.stderr[-4000:]}"


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("make") is None, reason="no hipcc")
@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_kernel_variant_type_checks(name):
    srcs = [f for f in os.listdir(CSRC) if f.endswith(".hip")]
    assert srcs
    for src in srcs:
        type_check(src, VARIANTS[name])


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("make") is None, reason="no hipcc")
def test_host_variant_type_checks():
    type_check("rrt_host.cpp", HOST_VARIANT)


def test_every_switch_is_compiled_at_a_non_default_value():
    """The module docstring, kept true: every `#ifndef RRT_X` switch under csrc/ is named by a variant's
    -D flag above or has a test of its own. A name check on preprocessor switches, nothing else."""
    switches = set()
    for f in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, f), encoding="utf-8", errors="replace") as fh:
            switches |= set(re.findall(r"#\s*ifndef\s+(RRT_\w+)", fh.read()))
    assert switches
    flags = [f for v in VARIANTS.values() for f in v] + HOST_VARIANT
    compiled = {re.match(r"-D(RRT_\w+)=", f).group(1) for f in flags}
    assert switches - compiled - TESTED_ELSEWHERE == set()
