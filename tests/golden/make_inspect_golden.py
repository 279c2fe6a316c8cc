#!/usr/bin/env python3
"""Generates tests/golden/ref_traverse_color.npz (run in the authoring container, where /root/reference is mounted, like make_golden.py):
GetTraverseCountColor of the reference's UNMODIFIED infra/helper.h, included by path and compiled with the flags of oracle/Makefile's `ref` target into a
temporary directory, evaluated on (traversed, peak) pairs.  The fixture is DATA (inputs + the three floats each); nothing compiled or copied from the
reference is kept."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("REF", "/root/reference")
REFCXX = os.environ.get("REFCXX", "/opt/rocm/lib/llvm/bin/clang++")
PEAKS = [0, 9, 10, 11, 57, 188, 255, 1000]
TRAVERSED = [-1, 0, 1, 5, 9, 10, 56, 57, 58, 500]

SRC = r"""
#include "precomp.h"
#include "helper.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv)
{
    for (int i = 1; i + 1 < argc; i += 2) {
        volatile int traversed = atoi(argv[i]), peak = atoi(argv[i + 1]);
        const float3 c = GetTraverseCountColor(traversed, peak);
        printf("%a %a %a\n", c.x, c.y, c.z);
    }
    return 0;
}
"""


def main():
    pairs = [(t, p) for p in PEAKS for t in TRAVERSED]
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "color.cpp"); exe = os.path.join(tmp, "color")
        open(src, "w").write(SRC)
        subprocess.check_call([REFCXX, "-std=c++17", "-O2", "-mavx2", "-ffp-contract=off", "-fms-extensions", "-w", "-Wno-non-pod-varargs", "-fno-access-control",
                               "-DGLFW_INCLUDE_NONE", "-I" + os.path.join(REPO, "oracle", "ref_build"), "-I" + REF + "/template", "-I" + REF + "/infra", "-I" + REF + "/lib",
                               "-I" + REF + "/lib/imgui", "-I" + REF + "/lib/GLFW/include", src, "-o", exe])
        out = subprocess.check_output([exe] + [str(v) for pr in pairs for v in pr], text=True)
    rgb = np.array([[float.fromhex(x) for x in line.split()] for line in out.strip().splitlines()], np.float32)
    assert rgb.shape == (len(pairs), 3)
    np.savez(os.path.join(HERE, "ref_traverse_color.npz"), traversed=np.array([p[0] for p in pairs], np.int32), peak=np.array([p[1] for p in pairs], np.int32), rgb=rgb)
    print("wrote ref_traverse_color.npz: %d pairs" % len(pairs))


if __name__ == "__main__":
    sys.exit(main())
