"""Conditions on tests/ray_query_cases.py, on the CPU: the scans that tests/test_gpu_ray_query.py
compares the query kernel with decide nearly every ray, every ray set both hits and misses, and the
record layouts are the header's.

Measured on the two scans alone (no kernel), RTOW: `camera` 1 ray of 4096 under (a) (it is under (c)
too: the ground sphere grazed), 1 under (b), 0.39 % under (c); `inside` 0 / 1 ray / 0.05 %. The Cornell
boxes' undecided rays are (b)'s: the light one unit under the ceiling, the faces' shared edges (0.2 to
0.8 %). The cap (2 %) is a condition on the ray sets, not a measurement of the kernel.
"""
import re
import os

import numpy as np
import pytest

from rustraytrace_amd import _lib

import ray_query_cases as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,ray_set,time", Q.CASES, ids=[f"{n}-{s}-{t:.2f}" for n, s, t in Q.CASES])
def test_scans_decide_and_sets_hit_and_miss(name, ray_set, time):
    sc = Q.case_scan(name, ray_set, time)
    n = len(sc.hit)
    frac = {k: float(v.mean()) for k, v in sc.reasons.items()}
    print(f"{name} {ray_set} t={time}: n={n} hits={sc.hit.mean():.3f} undecided={sc.undecided.mean():.4f} {frac}")
    assert n == Q.N_OF.get(name, Q.N_RAYS)
    assert sc.undecided.mean() <= Q.UNDECIDED_CAP
    assert sc.hit.mean() >= 0.10 and (~sc.hit).mean() >= 0.10


def test_record_layouts_match_the_header():
    assert _lib.RAY_DTYPE.itemsize == 32 and _lib.HIT_DTYPE.itemsize == 8
    assert _lib.RAY_DTYPE.names == ("o", "tmax", "d", "time")
    assert [_lib.RAY_DTYPE.fields[k][1] for k in _lib.RAY_DTYPE.names] == [0, 12, 16, 28]
    assert _lib.HIT_DTYPE.names == ("t", "prim") and [_lib.HIT_DTYPE.fields[k][1] for k in ("t", "prim")] == [0, 4]
    src = open(os.path.join(ROOT, "include", "rrt_hip.h")).read()
    ray = re.search(r"typedef struct RrtRay \{([^}]*)\}", src).group(1)
    assert re.findall(r"float (\w+)", ray) == ["o", "tmax", "d", "time"]
    hit = re.search(r"typedef struct RrtHit \{([^}]*)\}", src).group(1)
    assert re.findall(r"(?:float|uint32_t) (\w+)", hit) == ["t", "prim"]
    assert _lib.NO_PRIM == int(re.search(r"#define RRT_NO_PRIM (0x[0-9a-f]+)u", src).group(1), 16)
    assert _lib.QUERY_MODES == {"closest": 0, "any": 1}
    assert "RRT_QUERY_CLOSEST = 0, RRT_QUERY_ANY = 1" in src
