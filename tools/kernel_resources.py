"""The resource table of profiles/rNN_kernel_resources.txt: hipcc -Rpass-analysis=kernel-resource-usage (the Makefile's flags) for
every device translation unit of two source trees, the parent's and this one, kernel by kernel.

   python tools/kernel_resources.py <parent tree> [this tree, default .]  > profiles/rNN_kernel_resources.txt

`vs parent`: same = the line equals the parent's; moved = it differs without more spilled registers, more scratch or fewer
waves per SIMD (the parent's line follows in brackets); WORSE = it has one of those; new = a kernel the parent does not have.
rocPRIM's kernels are left out unless their lines differ."""
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

KEYS = ("VGPRs", "AGPRs", "TotalSGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")


def flags(root):
    text = open(os.path.join(root, "Makefile")).read()
    var = {n: re.search(rf"^{n}\s*[:?]?=\s*(.*)$", text, re.M).group(1).strip() for n in ("HIPCC", "ARCH", "NUMERICS", "HIPFLAGS")}
    return os.environ.get("HIPCC", var["HIPCC"]), var["HIPFLAGS"].replace("$(ARCH)", var["ARCH"]).replace("$(NUMERICS)", var["NUMERICS"]).split()


def usage(root, src, tmp):
    hipcc, fl = flags(root)
    p = subprocess.run([hipcc, *fl, "-S", "--cuda-device-only", "-o", os.path.join(tmp, "out.s." + str(abs(hash((root, src))))), src,
                        "-Rpass-analysis=kernel-resource-usage"], cwd=root, stderr=subprocess.PIPE, text=True)
    if p.returncode:
        raise RuntimeError(p.stderr[-2000:])
    out, name = {}, None
    for l in p.stderr.split("\n"):
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis", l)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            name = t.split(":", 1)[1].strip()
            out[name] = {}
        elif name and ": " in t:
            k, v = t.rsplit(": ", 1)
            out[name][k.strip()] = int(v) if v.isdigit() else v
    return out


def tree(root, tmp):
    srcs = sorted(glob.glob(os.path.join(root, "renderbaby_amd/csrc/*.hip")))
    with ThreadPoolExecutor(8) as ex:
        res = list(ex.map(lambda s: usage(root, os.path.relpath(s, root), tmp), srcs))
    return {(os.path.basename(s)[3:-4], k): v for s, r in zip(srcs, res) for k, v in r.items()}


def main():
    parent, child = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else ".")
    with tempfile.TemporaryDirectory() as tmp:
        a, b = tree(parent, tmp), tree(child, tmp)
    print(f"{'kernel':80s} " + " ".join(f"{h:>6s}" for h in ("VGPR", "AGPR", "SGPR", "vspill", "sspill", "scratc", "LDS", "occ")) + "  vs parent")
    worse = 0
    for (tu, k), v in b.items():
        line = [v.get(x, 0) for x in KEYS]
        old = a.get((tu, k))
        if old is None:
            tag = "new"
        else:
            ol = [old.get(x, 0) for x in KEYS]
            if ol == line:
                tag = "same"
            elif line[3] > ol[3] or line[4] > ol[4] or line[5] > ol[5] or line[7] < ol[7]:
                tag, worse = "WORSE [" + " ".join(map(str, ol)) + "]", worse + 1
            else:
                tag = "moved [" + " ".join(map(str, ol)) + "]"
        if "rocprim" in k and tag == "same":
            continue
        print(f"{(tu + ':' + k)[:80]:80s} " + " ".join(f"{x:6d}" for x in line) + "  " + tag)
    for key in a:
        if key not in b:
            print(f"{(key[0] + ':' + key[1])[:80]:80s} gone")
    print("worse:", worse)


if __name__ == "__main__":
    main()
