#!/usr/bin/env python3
"""Does the device code differ from a git revision's?  No GPU needed:
    python tools/isa_diff.py HEAD                     # every .hip of csrc/, the default build
    python tools/isa_diff.py HEAD --profile           # the -DGMR1_HIP_PROFILE build
    python tools/isa_diff.py HEAD rx_kernels.hip      # one translation unit
    python tools/isa_diff.py HEAD --resources k_rx4   # also the register/spill/LDS metadata of matching kernels, both sides
    python tools/isa_diff.py HEAD --rename ELi0EEEvNS_7PfbArgsE=EEEvNS_7PfbArgsE
                                                      # a kernel that gained a template parameter: its <..., 0> form is
                                                      # compared with REV's (a substring of the mangled name, new -> old)
csrc/ and include/ of REV are taken out of git into a temporary directory, every .hip of both trees is compiled to device-only
assembly with build.py's flags, and the output is compared kernel by kernel: the code from the kernel's symbol to the end of the
function, its .amdhsa_kernel block, its resource symbols and its metadata entry.  The assembly carries no file names or line
numbers, so a refactor that only moves text leaves it identical.  Prints the kernels that are new, gone or different (with both instruction counts)
and exits 1 if there are any.  What lies outside the kernels (constant tables, LDS symbols) is compared as one more entry."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "osmo-gmr_amd"
sys.path.insert(0, os.path.join(ROOT, PKG))
import build  # noqa: E402

JOBS = 16
REST = "(outside kernels)"
RES_KEYS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size")


def compile_asm(root, name, extra, out):
    """One .hip of the tree at `root` -> device assembly text."""
    flags = [f.replace(build.ROOT, root, 1) if f.startswith("-I") else f for f in build.COMMON]
    src = os.path.join(root, PKG, "csrc", name)
    p = subprocess.run([build.hipcc(), "-xhip"] + flags + extra + ["--offload-arch=" + build.ARCH, "--cuda-device-only", "-S",
                        src, "-o", out], capture_output=True, text=True)
    if p.returncode:
        raise RuntimeError("%s failed to compile:\n%s" % (src, p.stderr))
    return open(out).read()


def split_kernels(asm):
    """{symbol: text} per function (the kernels, and any device function left out of line) plus REST.  Block labels carry
    the function's index in the file (.LBB12_3) and the compilation unit's id hashes the source's path; both are dropped, so
    that neither a kernel added or removed nor the directory of the tree shows as a difference."""
    asm = re.sub(r"\.L(BB|func_end|func_begin)\d+", r".L\1", asm)
    asm = re.sub(r"\bBB\d+_", "BB_", asm)                     # ... and the loop comments that name a block
    asm = re.sub(r"[ \t]+;", " ;", asm)                       # (comments are aligned to a column: labels of other lengths shift them)
    asm = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", asm)
    cut = asm.find("amdhsa.kernels:")
    code, meta = (asm[:cut], asm[cut:]) if cut >= 0 else (asm, "")
    out, rest = {}, []
    pos = 0
    # a function: its "Begin function" line to "End function", the .set lines of its resource symbols and its info block
    fn = re.compile(r"^[^\n]*; -- Begin function (\S+)\n.*?; -- End function\n(?:\t\.set [^\n]*\n)*"
                    r"(?:\t\.section\t\.text\.[^\n]*\n)?(?:\t\.section\t\.AMDGPU\.csdata[^\n]*\n(?:;[^\n]*\n)*)?",
                    re.S | re.M)
    for m in fn.finditer(code):
        rest.append(code[pos:m.start()])
        out[m.group(1)] = m.group(0)
        pos = m.end()
    rest.append(code[pos:])
    for blk in re.split(r"^  - (?=\.agpr_count:)", meta, flags=re.M)[1:]:
        blk = blk.split("amdhsa.target:")[0]
        out[re.search(r"\.name:\s+(\S+)", blk).group(1)] += blk
    # (between functions only the switches back to a text section are left, which follow the functions' order)
    out[REST] = re.sub(r"^\t(\.text|\.section\t\.text\.[^\n]*)\n", "", "".join(rest), flags=re.M)
    return out


def n_insts(text):
    body = text.split("; -- End function")[0]
    return sum(1 for ln in body.split("\n") if ln.startswith("\t") and ln[1:2] not in (".", ";", ""))


def demangle(names):
    p = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return [re.sub(r"\(.*", "", n.replace("void ", "")) for n in p.stdout.split("\n")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("rev", help="git revision to compare the working tree against")
    ap.add_argument("files", nargs="*", help=".hip files of csrc/ (default: all of both trees)")
    ap.add_argument("--profile", action="store_true", help="compile with -DGMR1_HIP_PROFILE")
    ap.add_argument("--resources", metavar="KERNEL",
                    help="print the register, spill and LDS metadata of kernels whose name, demangled or mangled, contains KERNEL")
    ap.add_argument("--rename", metavar="NEW=OLD", action="append", default=[],
                    help="replace NEW by OLD in the working tree's assembly before comparing (mangled-name substrings)")
    a = ap.parse_args()
    extra = ["-DGMR1_HIP_PROFILE"] if a.profile else []
    with tempfile.TemporaryDirectory() as td:
        old = os.path.join(td, "old")
        os.mkdir(old)
        ar = subprocess.Popen(["git", "-C", ROOT, "archive", a.rev, PKG + "/csrc", "include"], stdout=subprocess.PIPE)
        subprocess.check_call(["tar", "-x", "-C", old], stdin=ar.stdout)
        if ar.wait():
            sys.exit("git archive %s failed" % a.rev)
        hips = lambda root: {f for f in os.listdir(os.path.join(root, PKG, "csrc")) if f.endswith(".hip") and (not a.files or f in a.files)}
        jobs = [(side, root, f) for side, root in (("old", old), ("new", ROOT)) for f in sorted(hips(root))]
        try:
            with ThreadPoolExecutor(JOBS) as ex:
                texts = list(ex.map(lambda j: compile_asm(j[1], j[2], extra, os.path.join(td, "%s_%s.s" % (j[0], j[2]))), jobs))
        except RuntimeError as e:
            sys.exit(str(e))
    kern = {"old": {}, "new": {}}
    for (side, _, f), t in zip(jobs, texts):
        for r in a.rename if side == "new" else ():
            t = t.replace(*r.split("=", 1))
        for sym, text in split_kernels(t).items():
            kern[side][(f, sym)] = text
    keys = sorted(set(kern["old"]) | set(kern["new"]))
    names = dict(zip(keys, demangle([k[1] for k in keys])))
    names.update({k: REST for k in keys if k[1] == REST})
    bad = 0
    for k in keys:
        o, n = kern["old"].get(k), kern["new"].get(k)
        if o == n:
            continue
        bad += 1
        if o is None or n is None:
            print("%-9s %s: %s" % ("new" if o is None else "gone", k[0], names[k]))
        else:
            print("different %s: %s  (%d -> %d instructions)" % (k[0], names[k], n_insts(o), n_insts(n)))
    if a.resources:
        for k in keys:
            if a.resources in names[k] or a.resources in k[1]:          # demangled or mangled
                for side in ("old", "new"):
                    t = kern[side].get(k, "")
                    print("%s %s: %s  %s" % (side, k[0], names[k], " ".join(
                        "%s=%s" % (r, m.group(1)) for r in RES_KEYS for m in [re.search(r"\.%s:\s+(\S+)" % r, t)] if m)))
    n_kern = sum(1 for t in kern["new"].values() if "\t.amdhsa_kernel " in t)
    print("%d kernels (%d entries with the out-of-line device functions and what lies outside) in %d files compared with %s: %s"
          % (n_kern, len(kern["new"]), len(hips(ROOT)), a.rev, "%d entries differ" % bad if bad else "identical"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
