#!/bin/bash
# Per-kernel ISA comparison of rrt_kernel.hip and rrt_books64.hip between a git revision and the
# working tree: device assembly of both with csrc/Makefile's flags, split per function, instruction
# lines compared (SAME / DIFF; block labels without their function number, which shifts when a
# function comes or goes).
#   tools/isa_diff.sh [REV=HEAD]
cd "$(dirname "$0")/.."
REV=${1:-HEAD}
T=$(mktemp -d)
# CXXFLAGS and KERNEL_FLAGS of csrc/Makefile; rrt_books64.hip takes -fno-slp-vectorize alone
CXX="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -fno-fast-math --cuda-device-only -S"
F_rrt_kernel="-fno-slp-vectorize -mllvm -amdgpu-sched-strategy=iterative-ilp -mllvm -structurizecfg-skip-uniform-regions=true"
F_rrt_books64="-fno-slp-vectorize"
mkdir -p $T/old/rustraytrace_amd/csrc $T/old/include
for f in rrt_kernel.hip rrt_books64.hip rrt_internal.h rrt_device.h rrt_box32.h rrt_sphere32.h; do
    git show $REV:rustraytrace_amd/csrc/$f > $T/old/rustraytrace_amd/csrc/$f
done
git show $REV:include/rrt_hip.h > $T/old/include/rrt_hip.h
for k in rrt_kernel rrt_books64; do
    flags=F_$k
    /opt/rocm/bin/hipcc $CXX ${!flags} $T/old/rustraytrace_amd/csrc/$k.hip -o $T/old_$k.s || exit 1
    /opt/rocm/bin/hipcc $CXX ${!flags} rustraytrace_amd/csrc/$k.hip -o $T/new_$k.s || exit 1
    echo "== $k.hip"
    python3 - $T/old_$k.s $T/new_$k.s <<'PY'
import re, sys
def funcs(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1); out[cur] = []
            continue
        if cur and line.startswith("\t.size\t" + cur):
            cur = None
            continue
        if cur and line.startswith("\t") and not line.startswith("\t.") and not line.startswith("\t;"):
            out[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0].strip()))
    return out
a, b = funcs(sys.argv[1]), funcs(sys.argv[2])
for k in sorted(set(a) | set(b)):
    s = "SAME" if a.get(k) == b.get(k) else "DIFF"
    print(s, len(a.get(k, [])), len(b.get(k, [])), k[:110])
PY
done
rm -rf $T
