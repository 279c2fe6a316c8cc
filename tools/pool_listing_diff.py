"""Are the kernels of a device file the same machine code in two builds?

    hipcc --offload-arch=gfx950 <the Makefile's CXXFLAGS and DEVFLAGS> --cuda-device-only -S -o a.s csrc/device/render_pool.hip      (one tree)
    ... -o b.s ...                                                                                                                   (the other)
    python tools/pool_listing_diff.py a.s b.s

once per file of the Makefile's SRC_DEV (and per diagnostic build, with its -D on both sides).  Compares every kernel of the two listings, keyed by its mangled
name — all instantiations of render_pool_kernel, and the kernels of the other device files alike — line by line: the instructions and the kernel descriptor
(the .amdhsa_* lines: registers, LDS, scratch).  What may differ and is normalised away: the ordinal of the function inside its file (the .LBB<n>_ label prefix)
and comments.  A kernel that only one listing has is a difference.  Prints one line per kernel and exits 1 on any difference, or when there is no kernel at all."""
import difflib
import re
import sys

NAME = re.compile(r"^([A-Za-z_$][\w$.]*):\s*; @")          # the label a function's body begins at


def bodies(path):
    out, cur = {}, None
    for line in open(path):
        line = line.rstrip("\n")
        m = NAME.match(line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        out[cur].append(line)
    return {k: v for k, v in out.items() if any(".amdhsa_kernel" in line for line in v)}       # kernels only: the descriptor lies inside the body


def normalised(name, body):
    res = []
    for line in body:
        line = line.split(";")[0].replace(name, "K")
        line = re.sub(r"\.LBB\d+_", ".LBB_", line).strip()
        if line:
            res.append(line)
    return res


def main(a, b):
    A, B = bodies(a), bodies(b)
    keys = sorted(set(A) | set(B))
    bad = 0
    for k in keys:
        if k not in A or k not in B:
            print("%s: missing in %s" % (k, b if k in A else a)); bad += 1; continue
        x, y = normalised(k, A[k]), normalised(k, B[k])
        same = x == y
        print("%s: %5d / %5d lines, %s" % (k, len(x), len(y), "identical" if same else "DIFFERENT"))
        if not same:
            bad += 1
            for d in list(difflib.unified_diff(x, y, lineterm="", n=0))[:40]:
                print("   ", d)
    print("%d kernels compared, %d differ" % (len(keys), bad))
    return 1 if bad or not keys else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
