"""Are the 16-bit-reference instantiations of render_pool_kernel the same machine code in two builds?

    hipcc --offload-arch=gfx950 <the Makefile's flags> --cuda-device-only -S -o a.s csrc/device/render_pool.hip      (one tree)
    ... -o b.s ...                                                                                                   (the other)
    python tools/pool_listing_diff.py a.s b.s

Compares the body of every render_pool_kernel<KIND, COUNT, S> (a tree without the width parameter) / <KIND, COUNT, S, 16> of the two listings, instruction by
instruction.  What may differ and is normalised away: the mangled name, the ordinal of the function inside its file (the .LBB<n>_ label prefix) and comments.
Prints one line per instantiation and exits 1 on any difference."""
import difflib
import re
import sys

NAME = re.compile(r"^(_ZN3crt18render_pool_kernelILi(\d)ELb(\d)ELi(\d+)E(?:Li(\d+)E)?EE\w*):")


def bodies(path):
    out, cur = {}, None
    for line in open(path):
        line = line.rstrip("\n")
        m = NAME.match(line)
        if m:
            cur = (m.group(2), m.group(3), m.group(4), m.group(5) or "16")
            out[cur] = (m.group(1), [])
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        out[cur][1].append(line)
    return out


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
    keys = sorted(k for k in A if k[3] == "16")
    bad = 0
    for k in keys:
        if k not in B:
            print(k, "missing in", b); bad += 1; continue
        x, y = normalised(*A[k]), normalised(*B[k])
        same = x == y
        print("KIND %s COUNT %s S %-3s: %5d / %5d lines, %s" % (k[0], k[1], k[2], len(x), len(y), "identical" if same else "DIFFERENT"))
        if not same:
            bad += 1
            for d in list(difflib.unified_diff(x, y, lineterm="", n=0))[:40]:
                print("   ", d)
    print("%d instantiations compared, %d differ" % (len(keys), bad))
    return 1 if bad or not keys else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
