"""CPU checks of the Whitted renderer's traversal inspection (crt_whitted_tick_inspect): the colour function's restatement against the reference's own
GetTraverseCountColor (tests/golden/ref_traverse_color.npz, written by tests/golden/make_inspect_golden.py from the unmodified infra/helper.h), the running
peak's semantics on a hand-made count image, declarations, exports, record size, NULL-context refusal, binding.  No compute call is made."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np

from conftest import GOLDEN, REPO
import inspect_restate as R


def test_restatement_equals_the_reference_colour_function():
    z = np.load(os.path.join(GOLDEN, "ref_traverse_color.npz"))
    assert len(z["peak"]) == 80 and set(z["peak"]) == {0, 9, 10, 11, 57, 188, 255, 1000} and set(z["traversed"]) == {-1, 0, 1, 5, 9, 10, 56, 57, 58, 500}
    got = R.traverse_count_color(z["traversed"], z["peak"])
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), z["rgb"].view(np.uint32))
    # blend == 1 is not `red` exactly: the arithmetic has to be kept operation for operation
    full = z["rgb"][(z["traversed"] == 500) & (z["peak"] == 57)][0]
    assert full[1] != np.float32(50) / np.float32(255) or full[2] != np.float32(50) / np.float32(255)


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(crt_[a-z_0-9]+)\s*\(", text))


def test_entries_declared_exported_and_listed(crt):
    lib = crt.lib()
    assert "crt_whitted_tick_inspect" in _declared("crt_abi.h") and "crt_whitted_tick_inspect" in crt.ABI_SYMBOLS and hasattr(lib, "crt_whitted_tick_inspect")
    for sym in ("crt_host_renderer_set_inspect", "crt_host_renderer_whitted_metrics"):
        assert sym in _declared("crt_host.h") and sym in crt.HOST_SYMBOLS and hasattr(lib, sym), sym
    assert lib.crt_abi_version() == 3
    text = open(os.path.join(REPO, "include", "crt_abi.h")).read()
    for name, val in (("CRT_INSPECT_NONE", 0), ("CRT_INSPECT_TRAVERSAL", 1), ("CRT_INSPECT_TESTS", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), text), name
    assert (crt.INSPECT_NONE, crt.INSPECT_TRAVERSAL, crt.INSPECT_TESTS) == (0, 1, 2)


def test_metrics_record_is_32_bytes(crt, tmp_path):
    assert C.sizeof(crt.WhittedMetricsS) == 32
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/llvm/bin/clang"
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include "crt_host.h"\n'
                   "_Static_assert(sizeof(crt_whitted_metrics) == 32, \"crt_whitted_metrics\");\n"
                   "_Static_assert(offsetof(crt_whitted_metrics, totalTests) == 16 && offsetof(crt_whitted_metrics, peakTests) == 28, \"layout\");\n")
    r = subprocess.run([cc, "-fsyntax-only", "-std=c11", "-I", os.path.join(REPO, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_context_is_refused_and_binding_exists(crt):
    L = crt.lib()
    m = crt.WhittedMetricsS()
    assert L.crt_whitted_tick_inspect(None, 0, 0, 0, None, None, None, C.byref(m)) == -1
    assert L.crt_host_renderer_set_inspect(None, 1, 0) == -1 and L.crt_host_renderer_whitted_metrics(None, C.byref(m), None, None) == -1
    assert callable(getattr(crt.Context, "whitted_tick_inspect", None))
    assert callable(getattr(crt.HostRenderer, "set_inspect", None)) and callable(getattr(crt.HostRenderer, "whitted_metrics", None))


def test_running_peak_on_a_hand_made_image():
    green = np.array(R.GREEN, np.float32)
    #                 0  1  2  3   4   5   6   7   8   9  10  11
    count = np.array([[3, 9, 0, 7, 12, 6, 12, 30, 15, 30, 4, 20]], np.int32).reshape(3, 4)
    hit = np.ones((3, 4), bool); hit[0, 2] = False
    sky = np.zeros((3, 4, 4), np.float32); sky[..., :3] = np.float32(0.25)
    acc, screen, peak_out, peaks = R.heat_map(count, hit, sky, 0)
    flat = acc.reshape(-1, 4); pk = peaks.ravel()
    assert list(pk) == [0, 3, 9, 9, 9, 12, 12, 12, 30, 30, 30, 30] and peak_out == 30
    # the leading run stays green: the peak is under 10 up to and INCLUDING the pixel that raises it to 12 (it is coloured with the previous peak, 9)
    for i in (0, 1, 3, 4):
        assert np.array_equal(flat[i, :3].view(np.uint32), green.view(np.uint32)), i
    assert np.array_equal(flat[2], sky[0, 2])                                        # a miss is the sky, and still raises nothing here (count 0)
    assert np.all(flat[:, 3] == 0)
    # pixel 7 (30 > peakIn 12 >= 10) is clamped: blend == 1, red by formula (not the constant)
    by_formula = R.traverse_count_color(np.array([12]), np.array([12]))[0]
    assert np.array_equal(flat[7, :3].view(np.uint32), by_formula.view(np.uint32)) and flat[7, 0] == np.float32(1)
    assert np.array_equal(flat[6, :3].view(np.uint32), by_formula.view(np.uint32))    # 12 of 12
    assert np.array_equal(flat[5, :3].view(np.uint32), R.traverse_count_color(np.array([6]), np.array([12]))[0].view(np.uint32))
    assert np.array_equal(flat[8, :3].view(np.uint32), R.traverse_count_color(np.array([15]), np.array([30]))[0].view(np.uint32))
    # a second Tick with the returned peak: the global maximum everywhere
    acc2, _, peak2, peaks2 = R.heat_map(count, hit, sky, peak_out)
    assert peak2 == 30 and np.all(peaks2 == 30)
    want = R.traverse_count_color(count, np.full(count.shape, 30))
    assert np.array_equal(acc2[..., :3][hit].view(np.uint32), want[hit].view(np.uint32))
    assert np.array_equal(screen[0, 2], R.rgb8(sky[0, 2, :3]))
    m = R.metrics(count, count * 2, 0, 100)
    assert m == dict(rayHitCount=11, totalTraversal=148, totalTests=296, peakTraversal=30, peakTests=100)
