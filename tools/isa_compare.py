"""Compare the gfx950 device code of two builds of the library's sources, kernel by kernel.

For each source file, both trees are compiled with build.py's flags plus `--cuda-device-only -S
-Rpass-analysis=kernel-resource-usage` (no GPU needed).  A kernel's instructions are the lines of its body up to its
.Lfunc_end label, directives and comments dropped, local labels normalised; IDENTICAL = the same instruction text.  The
resource-usage remarks give VGPRs, LDS, scratch and occupancy per kernel.  Kernels only in the new build are listed as
added; a kernel of the base build that is missing (with the base build's figures, for a kernel that moved or was
renamed) or differs is reported, and the exit status is 1.  A file that only one tree has counts as one without kernels.

usage: python tools/isa_compare.py BASE_TREE NEW_TREE file.hip [file.hip ...] [--out report.txt]"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from descriptools_amd.build import FLAGS  # noqa: E402

LABEL = re.compile(r"\.L[A-Za-z_]*\d+(_\d+)?")


def compile_asm(tree, src, out_dir):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    s = os.path.join(out_dir, os.path.basename(src) + ".s")
    if not os.path.exists(os.path.join(tree, "descriptools_amd", "csrc", src)):
        return "", ""
    flags = [f for f in FLAGS if f not in ("-fPIC", "-Wall")]
    r = subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                                          os.path.join(tree, "descriptools_amd", "csrc", src), "-o", s],
                       capture_output=True, text=True, check=True)
    return open(s).read(), r.stderr


def kernels(asm):
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
    out = {}
    for n in names:
        m = re.search(r"^" + re.escape(n) + r":.*?$(.*?)^\.Lfunc_end", asm, re.M | re.S)
        body = []
        for line in m.group(1).splitlines():
            t = line.split(";")[0].strip()
            if not t or t.startswith(".") or t.endswith(":"):
                continue
            body.append(LABEL.sub(".L", t))
        out[n] = body
    return out


def resources(remarks):
    res, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|LDS Size \[bytes/block\]|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]):"
                      r" (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split()[0]] = int(m.group(2))
    return res


def main():
    args = sys.argv[1:]
    out_path = None
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    base, new, files = args[0], args[1], args[2:]
    lines, bad = [], 0
    with tempfile.TemporaryDirectory() as tb, tempfile.TemporaryDirectory() as tn:
        for f in files:
            a_asm, a_rem = compile_asm(base, f, tb)
            b_asm, b_rem = compile_asm(new, f, tn)
            ka, kb = kernels(a_asm), kernels(b_asm)
            ra, rb = resources(a_rem), resources(b_rem)
            added = sorted(set(kb) - set(ka))
            lines.append("%s: kernels in base %d, in this change %d, added %s" % (f, len(ka), len(kb), added))
            for n in sorted(ka):
                if n not in kb:
                    r = ra.get(n, {})
                    lines.append("  MISSING   %-70s instr %5d        VGPRs %3s LDS %6s B scratch %s waves/SIMD %s" % (
                        n, len(ka[n]), r.get("VGPRs"), r.get("LDS"), r.get("ScratchSize"), r.get("Occupancy")))
                    bad += 1
                    continue
                same = ka[n] == kb[n]
                rsame = ra.get(n) == rb.get(n)
                bad += (not same) + (not rsame)
                r = rb.get(n, {})
                lines.append("  %-9s %-70s instr %5d %5d  VGPRs %3s LDS %6s B scratch %s waves/SIMD %s%s" % (
                    "IDENTICAL" if same else "DIFFERENT", n, len(ka[n]), len(kb[n]), r.get("VGPRs"), r.get("LDS"),
                    r.get("ScratchSize"), r.get("Occupancy"), "" if rsame else "  (resources differ: %s)" % ra.get(n)))
            for n in added:
                r = rb.get(n, {})
                lines.append("  new       %-70s instr       %5d  VGPRs %3s LDS %6s B scratch %s waves/SIMD %s" % (
                    n, len(kb[n]), r.get("VGPRs"), r.get("LDS"), r.get("ScratchSize"), r.get("Occupancy")))
    lines.append("base kernels that differ or are missing: %d" % bad)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
