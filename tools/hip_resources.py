#!/usr/bin/env python3
"""Per kernel instance of one csrc/*.hip file, from the compiler's own remarks (no GPU needed): VGPRs, AGPRs, SGPRs, scratch, LDS and
occupancy for gfx950, as a CSV.  An instance with scratch_bytes > 0 spills.

    python tools/hip_resources.py bot_amd/csrc/spmm_rel.hip > profiles/spmm_rel_resources.csv"""
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
if len(sys.argv) != 2 or not os.path.isfile(sys.argv[1]):
    sys.exit("usage: python tools/hip_resources.py <bot_amd/csrc/FILE.hip>   (the CSV goes to standard output)")
src = sys.argv[1]
with tempfile.TemporaryDirectory() as tmp:
    err = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                          os.path.join(tmp, "o.o")], capture_output=True, text=True, check=True).stderr
rows = []
for block in re.split(r"remark: [^\n]*Function Name: ", err)[1:]:
    get = lambda key: int(re.search(key + r": (\d+)", block).group(1))
    rows.append((block.split("\n")[0].strip(), get("VGPRs"), get("AGPRs"), get("SGPRs"), get(r"ScratchSize \[bytes/lane\]"),
                 get(r"LDS Size \[bytes/block\]"), get(r"Occupancy \[waves/SIMD\]")))
names = subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True, text=True, check=True).stdout.split("\n")
print("kernel,vgpr,agpr,sgpr,scratch_bytes,lds_bytes,occupancy")
for name, r in sorted((n.replace("void ", "").split("(")[0], r) for n, r in zip(names, rows)):
    print('"%s",%d,%d,%d,%d,%d,%d' % ((name,) + r[1:]))
