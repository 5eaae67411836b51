"""Register and scratch budgets of every kernel instantiation, against the parent's.

The kernel sources are compiled for gfx950 with the flags `make resource` uses (read from the
Makefile by `make -n resource`, device side only) and -Rpass-analysis=kernel-resource-usage. Every
rrt_render / rrt_render64 instantiation is held to tests/golden/kernel_resources_parent.json, the
table the same command gave at the parent of the change that took the f32 path throughput out of
scratch: no instantiation may ask for more VGPRs, spill more VGPRs or SGPRs, or use more scratch.
C2's kernel, rrt_render<true, false, uint16_t, false, 8, -1, 1024, false>, is held to the figure that
change reached (C2_KERNEL below).

The table belongs to one compiler: the tests skip when `hipcc --version` is not the recorded one.
Regenerate (at the commit whose figures are to be the table):
    python tests/test_kernel_resources.py tests/golden/kernel_resources_parent.json
CPU only: hipcc cross-compiles without a GPU.
"""
import json
import os
import re
import shlex
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rustraytrace_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_resources_parent.json")

C2_NAME = "_ZN3rrt12_GLOBAL__N_110rrt_renderILb1ELb0EtLb0ELi8ELin1ELi1024ELb0EEEvNS_7KParamsE"
# the figure reached: 64 VGPRs at 8 waves/SIMD, no scratch, nothing spilled
C2_KERNEL = {"vgprs": 64, "occupancy": 8, "scratch": 0, "vgpr_spill": 0, "sgpr_spill": 0}

FIELDS = {
    "TotalSGPRs": "sgprs",
    "VGPRs": "vgprs",
    "AGPRs": "agprs",
    "ScratchSize [bytes/lane]": "scratch",
    "Occupancy [waves/SIMD]": "occupancy",
    "SGPRs Spill": "sgpr_spill",
    "VGPRs Spill": "vgpr_spill",
}
# what no instantiation may raise
HELD = ("vgprs", "vgpr_spill", "sgpr_spill", "scratch")


def hipcc_version():
    """The HIP version and clang version lines of `hipcc --version` (not the install paths)."""
    out = subprocess.run([HIPCC, "--version"], capture_output=True, text=True, timeout=60).stdout
    return "\n".join(l.strip() for l in out.splitlines() if l.startswith("HIP version") or "clang version" in l)


def resource_commands():
    """`make resource`'s compile lines, as argument lists, device side only, output to `out`."""
    r = subprocess.run(["make", "-n", "-C", CSRC, "resource"], capture_output=True, text=True, timeout=60, check=True)
    cmds = []
    for line in r.stdout.splitlines():
        if "-Rpass-analysis=kernel-resource-usage" not in line:
            continue
        args = shlex.split(line)
        assert args[0].endswith("hipcc") and "-o" in args, line
        cmds.append(args)
    assert len(cmds) == 2, r.stdout
    return cmds


def parse_remarks(text):
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = out.setdefault(val, {})
        elif cur is not None and key in FIELDS:
            cur[FIELDS[key]] = int(val)
    return out


def compile_one(args, tmp):
    args = list(args)
    args[args.index("-o") + 1] = os.path.join(tmp, "k.o")
    args += ["--cuda-device-only", "-Wno-unused-command-line-argument"]
    r = subprocess.run(args, cwd=CSRC, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-4000:]
    return parse_remarks(r.stderr)


def collect():
    cmds = resource_commands()
    table = {}
    with tempfile.TemporaryDirectory() as t0, tempfile.TemporaryDirectory() as t1:
        with ThreadPoolExecutor(2) as ex:
            for part in ex.map(compile_one, cmds, (t0, t1)):
                table.update(part)
    return table


@pytest.fixture(scope="module")
def tables():
    if not os.path.exists(HIPCC) or shutil.which("make") is None:
        pytest.skip("no hipcc")
    golden = json.load(open(GOLDEN))
    if hipcc_version() != golden["hipcc_version"]:
        pytest.skip("hipcc is not the compiler the table was recorded with")
    return golden["kernels"], collect()


def render_kernels(table):
    return sorted(k for k in table if re.search(r"\d+rrt_render(64)?I", k))


def test_table_covers_the_render_kernels(tables):
    parent, new = tables
    assert len(render_kernels(parent)) > 100 and C2_NAME in parent
    assert render_kernels(new) == render_kernels(parent)


def test_no_instantiation_asks_for_more(tables):
    parent, new = tables
    worse = []
    for k in render_kernels(parent):
        for f in HELD:
            if new[k][f] > parent[k][f]:
                worse.append(f"{k}: {f} {parent[k][f]} -> {new[k][f]}")
    assert not worse, "\n".join(worse)


def test_c2_kernel_holds_its_path_state_in_registers(tables):
    _, new = tables
    got = {f: new[C2_NAME][f] for f in C2_KERNEL}
    print(got)
    assert got == C2_KERNEL


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump({"hipcc_version": hipcc_version(), "kernels": collect()}, f, indent=0, sort_keys=True)
        f.write("\n")
