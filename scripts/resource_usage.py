#!/usr/bin/env python3
"""Per-kernel resource usage of HIP sources (VGPRs, spills, LDS, occupancy),
from hipcc's -Rpass-analysis=kernel-resource-usage remarks.  Host-side tool.

    python scripts/resource_usage.py SOURCE.hip [SOURCE.hip ...] [filter [hipcc flags...]]

Several sources print one table, e.g. the plain plane-march predictor
(fields3d.hip) next to its buoyant instantiations (buoyancy3d.hip):

    python scripts/resource_usage.py cfd-simulations_amd/csrc/fields3d.hip \
        cfd-simulations_amd/csrc/buoyancy3d.hip k_predictor3d_planes

whose names read k_predictor3d_planes<VEC, R, SUPG, NM, ZPER, BUOY> (NM: 0
scalar, 1 array, 2 LES); k_predictor3d<SUPG, NM, ZP, ...> with a trailing
cfd::Pred3Buoy is the buoyant per-cell kernel.
"""
import re
import subprocess
import sys
import tempfile

args = sys.argv[1:]
srcs = []
while args and args[0].endswith(".hip"):
    srcs.append(args.pop(0))
if not srcs:
    sys.exit(__doc__)
flt = args[0] if args else ""
extra = args[1:]
rows = []
for src in srcs:
    with tempfile.NamedTemporaryFile(suffix=".o") as obj:
        out = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950",
                              "-ffp-contract=off", "-c", src, "-o", obj.name,
                              "-Rpass-analysis=kernel-resource-usage", *extra], capture_output=True, text=True).stderr
    cur = None
    for line in out.splitlines():
        m = re.search(r"remark: (?:\s*)(Function Name|VGPRs|VGPRs Spill|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]|SGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]): (\S+)", line)
        if not m:
            continue
        k, v = m.group(1), m.group(2)
        if k == "Function Name":
            cur = {"name": subprocess.run(["c++filt", v], capture_output=True, text=True).stdout.strip()}
            rows.append(cur)
        elif cur is not None:
            cur[k.split(" ")[0] + ("_spill" if "Spill" in k else "")] = v
for r in rows:
    if flt in r["name"]:
        print(f'{r.get("VGPRs","?"):>4} vgpr {r.get("VGPRs_spill","?"):>3} spill {r.get("TotalSGPRs","?"):>4} sgpr '
              f'{r.get("ScratchSize","?"):>3} scratch {r.get("LDS","?"):>6} lds '
              f'occ {r.get("Occupancy","?")}  {r["name"][:150]}')
