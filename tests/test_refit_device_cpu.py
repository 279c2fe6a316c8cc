"""crt_refit_device / crt_host_scene_bvh_refit_device (BVH::Refit on the device from positions in device memory) — what runs without a GPU: the entries are
exported and listed, the header declares them without a new ABI version, and a NULL context is refused before anything touches a device.  The stale-mark rules
of the host front need a refit to have happened, so they are checked on the device (tests/test_gpu_refit_device.py)."""
import ctypes as C
import os
import re

from conftest import REPO

ENTRIES = ("crt_refit_device", "crt_host_scene_bvh_refit_device")


def test_entries_are_exported_and_listed(crt):
    L = crt.lib()
    assert "crt_refit_device" in crt.ABI_SYMBOLS and "crt_host_scene_bvh_refit_device" in crt.HOST_SYMBOLS
    for name in ENTRIES:
        assert getattr(L, name) is not None
    assert callable(crt.Context.refit_device) and callable(crt.HostScene.refit_device)


def test_header_declares_the_entry_and_keeps_the_abi_version(crt):
    abi = open(os.path.join(REPO, "include", "crt_abi.h")).read()
    host = open(os.path.join(REPO, "include", "crt_host.h")).read()
    assert re.search(r"int\s+crt_refit_device\s*\(\s*crt_ctx\s*\*\s*ctx\s*,\s*uint32_t\s+bvh\s*,\s*const\s+float\s*\*\s*d_positions", abi)
    assert re.search(r"int\s+crt_host_scene_bvh_refit_device\s*\(", host)
    assert re.search(r"#define\s+CRT_ABI_VERSION\s+3\b", abi)
    assert crt.lib().crt_abi_version() == 3


def test_null_context_is_invalid(crt):
    L = crt.lib()
    pos = (C.c_float * 9)()
    box = (C.c_float * 6)()
    assert L.crt_refit_device(None, C.c_uint32(0), pos, C.c_uint32(1), None, box) == -1                 # CRT_ERR_INVALID
    assert L.crt_host_scene_bvh_refit_device(None, None, 0, pos, C.c_uint32(1), None) == -1
