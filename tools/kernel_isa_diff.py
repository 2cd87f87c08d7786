"""Per-kernel ISA comparison of one HIP source between a git revision and the working tree.

    python tools/kernel_isa_diff.py REV csrc/plant.hip [kernel ...]

Compiles the file at REV (with REV's headers) and in the working tree with the library's
flags and ``-S --cuda-device-only``, cuts each named kernel's body out of the two listings
(from its label to its function end), drops comments and blank lines, renumbers the local
labels in order of appearance (new kernels in the file shift the compiler's numbering) and
prints ``diff`` of the two: empty when the kernel is the same instruction for instruction.
With no kernel named, every kernel of either listing is compared (their
``.amdhsa_kernel NAME`` directives list them, by mangled name).  Exit status 1 if any kernel
differs or is missing on either side.
"""
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "senquential-convex-programming-for-trajectory-planning_amd"
sys.path[:0] = [os.path.join(ROOT, PKG)]

from scpqp.build import ARCH  # noqa: E402


def listing(tree, rel, out):
    subprocess.run(["hipcc", "-S", "--cuda-device-only", "--offload-arch=" + ARCH, "-O3", "-std=c++17",
                    "-fPIC", "-Wno-unused-result", "-Wno-unused-command-line-argument",
                    "-I" + os.path.join(tree, "include"), os.path.join(tree, PKG, rel), "-o", out],
                   check=True)
    return open(out).read().splitlines()


def kernels_of(lines):
    """The mangled names of the listing's kernels, in order."""
    return [ln.split()[1] for ln in lines if ln.strip().startswith(".amdhsa_kernel ")]


def body(lines, kernel):
    """The instruction lines of the kernel whose mangled name is `kernel` or holds
    <len><kernel>E."""
    if kernel.startswith("_Z"):
        tag = re.compile(r"^(%s):" % re.escape(kernel))
    else:
        tag = re.compile(r"^(_Z\w*?%d%sE\w*):" % (len(kernel), re.escape(kernel)))
    out, on = [], False
    for ln in lines:
        if not on and tag.match(ln):
            on = True
        if on:
            if ln.startswith(".Lfunc_end"):
                break
            code = ln.split(";", 1)[0].rstrip()
            if code.strip():
                out.append(code)
    names = {}
    return [re.sub(r"\.L\w+", lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), ln)
            for ln in out]


def main():
    rev, rel, kernels = sys.argv[1], sys.argv[2], sys.argv[3:]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        old = os.path.join(tmp, "old")
        os.makedirs(old)
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "include", PKG + "/csrc"],
                             check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", old], input=tar, check=True)
        a = listing(old, rel, os.path.join(tmp, "old.s"))
        b = listing(ROOT, rel, os.path.join(tmp, "new.s"))
    if not kernels:
        kernels = list(dict.fromkeys(kernels_of(a) + kernels_of(b)))
    for k in kernels:
        x, y = body(a, k), body(b, k)
        print(f"$ diff <(kernel_body {rev}:{rel} {k}) <(kernel_body worktree:{rel} {k})")
        d = list(difflib.unified_diff(x, y, lineterm="", n=0))
        if not x or not y or d:
            bad += 1
            print("\n".join(d) if x and y else f"kernel {k} not found ({len(x)} / {len(y)} lines)")
        else:
            print(f"(empty: {len(x)} lines identical)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
