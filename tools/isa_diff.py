"""Did a kernel refactor change an instruction?  Compile every source of the library from two trees to gfx950 assembly
and compare the text.

    python tools/isa_diff.py <tree A> <tree B> [source.hip ...]

Each entry of build.SOURCES (or the sources named) is compiled from both trees with the library's own flags
(audiocaption_amd.build of the tree this tool lives in) plus ``-x hip --cuda-device-only -S``, from inside the tree's csrc
directory so that no path reaches the output.  The only lines dropped are those carrying the per-compilation
``__hip_cuid_...`` symbol; everything else - instructions, labels, the register / LDS / scratch figures of every
kernel descriptor - is compared as whole text.  Prints ``identical`` or the first differing line and the kernel it
belongs to, per source; exits 1 if anything differed.  Needs hipcc, no GPU.
"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audiocaption_amd import build  # noqa: E402

KERNEL = re.compile(r"^\s*\.(?:type\s+(\S+),@function|amdhsa_kernel\s+(\S+))")


def assembly(tree, src, out_dir):
    csrc = os.path.join(os.path.abspath(tree), "audiocaption_amd", "csrc")
    out = os.path.join(out_dir, src.replace(".hip", ".s"))
    cmd = [build._hipcc(), "-x", "hip", "--cuda-device-only", "-S", src, "-o", out]
    cmd += build.FLAGS + build.NO_PACKED_F32 + build.EXTRA_FLAGS.get(src, [])
    r = subprocess.run(cmd, cwd=csrc, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {tree}: {src}\n{r.stdout.decode()}")
    with open(out) as f:
        return [line.rstrip("\n") for line in f if "__hip_cuid_" not in line]


def first_difference(a, b):
    """None, or (kernel, line number, line of a, line of b) at the first line that differs."""
    kernel = "(before the first kernel)"
    for i in range(max(len(a), len(b))):
        la = a[i] if i < len(a) else "<end of file>"
        lb = b[i] if i < len(b) else "<end of file>"
        if la != lb:
            return kernel, i + 1, la, lb
        m = KERNEL.match(la)
        if m:
            kernel = m.group(1) or m.group(2)
        elif la.lstrip().startswith(".end_amdhsa_kernel"):
            kernel = f"(after {kernel}: that kernel and its descriptor are identical)"
    return None


def main(argv):
    if len(argv) < 2:
        print(__doc__)
        return 2
    tree_a, tree_b, sources = argv[0], argv[1], argv[2:] or build.SOURCES
    differing = 0
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(8) as pool:
        dirs = [os.path.join(tmp, d) for d in ("a", "b")]
        for d in dirs:
            os.mkdir(d)
        jobs = [(src, pool.submit(assembly, tree_a, src, dirs[0]), pool.submit(assembly, tree_b, src, dirs[1]))
                for src in sources]
        for src, fa, fb in jobs:
            a, b = fa.result(), fb.result()
            diff = first_difference(a, b)
            if diff is None:
                print(f"{src:26s} identical ({len(a)} lines)")
            else:
                differing += 1
                kernel, line, la, lb = diff
                print(f"{src:26s} DIFFERS first in {kernel}, line {line} ({len(a)} vs {len(b)} lines)\n    A: {la.strip()}\n    B: {lb.strip()}")
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
