"""Memory loads left inside the factorisation's and the triangular solves' loops, and the
dynamic-LDS offset-table lookups per function, from the ISA of one kernel group (no GPU).

    python tools/isa_loop_loads.py GROUP [REV]

Compiles csrc/kernels.hip for kernel group GROUP (the library's flags, ``-S
--cuda-device-only -gline-tables-only``; the line tables do not change the code) from the
working tree, or from git revision REV (with REV's headers), and prints

* per function, the number of ``llvm.amdgcn.dynlds.offset.table`` address formations (one per
  lookup of the dynamic LDS base; a function of the kernel that names ``smem_`` pays one per
  reference, and again after barriers) and the function's instruction count;
* every ``global_load*`` / ``s_load*`` / ``s_buffer_load*`` / ``scratch_load*`` that sits
  inside a loop (between a label and a later branch back to it) and whose source position, or
  the position of any frame it was inlined into, lies in ``panel_factor`` .. ``cholesky`` or
  in ``Solver`` .. ``chol_solve`` of scpqp_kernel.h.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "senquential-convex-programming-for-trajectory-planning_amd"
sys.path[:0] = [os.path.join(ROOT, PKG)]

from scpqp.build import ARCH  # noqa: E402

TABLE = "llvm.amdgcn.dynlds.offset.table@rel32@lo"
LOADS = re.compile(r"^\s*(global_load\w*|s_load\w*|s_buffer_load\w*|scratch_load\w*|flat_load\w*)\s")


def source_ranges(header):
    """{name: (first line, last line)} of the factorisation and of the triangular solves."""
    lines = open(header).read().splitlines()

    def at(pat, start=0):
        for i in range(start, len(lines)):
            if re.search(pat, lines[i]):
                return i + 1
        raise ValueError(pat)

    def end_of(first):   # the closing brace in column 0 after `first`
        return at(r"^}", first)

    pf = at(r"void panel_factor\(") - 1
    ch = at(r"__device__ bool cholesky\(")
    so = at(r"^struct Solver")
    cs = at(r"void chol_solve\(")
    return {"factor": (pf, end_of(ch)), "solve": (so - 1, end_of(cs))}


def listing(tree, group, out):
    subprocess.run(["hipcc", "-S", "--cuda-device-only", "--offload-arch=" + ARCH, "-O3", "-std=c++17",
                    "-fPIC", "-gline-tables-only", "-Wno-unused-result",
                    "-Wno-unused-command-line-argument", "-DSCPQP_KGROUP=%d" % group,
                    "-I" + os.path.join(tree, "include"),
                    os.path.join(tree, PKG, "csrc", "kernels.hip"), "-o", out], check=True)
    return open(out).read().splitlines()


def functions(lines):
    """[(mangled name, [(instruction text, [source lines of its inline chain])])]"""
    res, cur, chain = [], None, []
    for ln in lines:
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            cur = []
            res.append((m.group(1), cur))
            continue
        if cur is None:
            continue
        if ln.startswith(".Lfunc_end"):
            cur = None
            continue
        s = ln.strip()
        if s.startswith(".loc"):
            # .loc F L C ... ; file:L:C @[ file:L:C @[ ... ] ]   (only scpqp_kernel.h frames count)
            com = ln.split(";", 1)[1] if ";" in ln else ""
            chain = [int(x) for x in re.findall(r"scpqp_kernel\.h:(\d+):\d+", com)]
            continue
        if not s or s.startswith((";", ".")) and not s.startswith(".LBB"):
            continue
        cur.append((ln.split(";", 1)[0].rstrip(), chain))
    return res


def in_loops(body):
    """Indices of the instructions that lie between a label and a later branch to it."""
    label = {}
    inside = set()
    for i, (t, _) in enumerate(body):
        m = re.match(r"^(\.LBB\w+):", t)
        if m:
            label[m.group(1)] = i
        m = re.match(r"^\s*s_c?branch\w*\s+(\.LBB\w+)", t)
        if m and m.group(1) in label:
            inside.update(range(label[m.group(1)], i + 1))
    return inside


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True,
                         text=True).stdout.splitlines()
    return [(re.search(r"(\w+)<", d) or re.search(r"(\w+)\(", d) or re.match(r"(.*)", d)).group(1) for d in out]


def main():
    group = int(sys.argv[1])
    rev = sys.argv[2] if len(sys.argv) > 2 else None
    with tempfile.TemporaryDirectory() as tmp:
        tree = ROOT
        if rev:
            tree = os.path.join(tmp, "rev")
            os.makedirs(tree)
            tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "include", PKG + "/csrc"],
                                 check=True, capture_output=True).stdout
            subprocess.run(["tar", "-x", "-C", tree], input=tar, check=True)
        rng = source_ranges(os.path.join(tree, PKG, "csrc", "scpqp_kernel.h"))
        fns = functions(listing(tree, group, os.path.join(tmp, "k.s")))
    print(f"# kernel group {group}, {rev or 'working tree'}; source ranges {rng}")
    print("# function: offset-table lookups / instructions")
    total = 0
    for (name, body), short in zip(fns, demangle([n for n, _ in fns])):
        insts = [t for t, _ in body if not re.match(r"^\.LBB", t)]
        n = sum(TABLE in t for t in insts)
        total += n
        print(f"{short:32s} {n:3d} / {len(insts)}")
    print(f"total offset-table lookups: {total}")
    print("# loads inside loops of the factorisation (factor) and the triangular solves (solve)")
    left = 0
    for (name, body), short in zip(fns, demangle([n for n, _ in fns])):
        loop = in_loops(body)
        for i, (t, chain) in enumerate(body):
            if i not in loop or not LOADS.match(t):
                continue
            for what, (a, b) in rng.items():
                if any(a <= ln <= b for ln in chain):
                    left += 1
                    print(f"{short:32s} {what:6s} line {chain[0]:4d}  {t.strip()}")
                    break
    print(f"loads left in those loops: {left}")


if __name__ == "__main__":
    main()
