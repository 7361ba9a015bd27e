"""Kernel resource table (VGPR/AGPR/SGPR/scratch/occupancy/LDS, VGPR and SGPR spills) for every k_* instantiation, from hipcc's
-Rpass-analysis=kernel-resource-usage remarks (device-only compile, no GPU needed).
usage: python tools/kernel_resources.py [filter-substring] [--remarks=FILE] [extra hipcc flags...]
(--remarks=FILE: read the remarks of an earlier compile -- hipcc's stderr, as loop_spill_traffic.py --remarks-out=FILE keeps it --
instead of compiling again)"""
import os, re, subprocess, sys
HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "..", "roborugby_amd", "csrc", "rr_kernels.hip")
flt = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else ""
saved = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--remarks=")]
extra = [a for a in sys.argv[1:] if a.startswith("-") and not a.startswith("--remarks=")]
cmd = ["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "--offload-device-only", "-c",
       "-Rpass-analysis=kernel-resource-usage", "-o", "/tmp/rr_kres.o", SRC] + extra
out = open(saved[0]).read() if saved else subprocess.run(cmd, capture_output=True, text=True).stderr
rows, cur = [], None
for line in out.splitlines():
    m = re.search(r"remark:\s+(.*?):\s*(.*?) \[-Rpass", line)
    if not m: continue
    k, v = m.group(1).strip(), m.group(2).strip()
    if k == "Function Name":
        name = subprocess.run(["c++filt", v], capture_output=True, text=True).stdout.strip()
        cur = {"name": name}; rows.append(cur)
    elif cur is not None: cur[k] = v
for r in rows:
    m = re.match(r"void (\w+)<rr::Cfg<(\d+), (\d+), (\d+), (\d+), (?:rr::)?(\w+), (\d+)>(?:, (\w+))?(?:, (\w+))?(?:, (\w+))?>", r["name"])
    tag = r["name"][:60] if not m else "%s %s+%s/%s+%s %s VW%s out=%s multi=%s budget=%s" % m.groups()
    if flt and flt not in tag: continue
    # spillS: scalar registers the allocator parked in lanes of a VGPR (every use is a v_readlane + hazard slot: loop_spill_traffic.py)
    print("%-72s vgpr %3s agpr %3s sgpr %3s scratch %4s occ %s spillV %3s spillS %3s lds %6s" % (tag, r.get("VGPRs"), r.get("AGPRs"),
          r.get("TotalSGPRs"), r.get("ScratchSize [bytes/lane]"), r.get("Occupancy [waves/SIMD]"), r.get("VGPRs Spill"), r.get("SGPRs Spill"),
          r.get("LDS Size [bytes/block]")))
