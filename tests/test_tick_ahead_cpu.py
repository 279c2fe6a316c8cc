"""crt_tick without a GPU: the entry point is declared, exported, wrapped by the binding, and refuses a NULL context."""
import ctypes as C
import os

from conftest import REPO


def test_crt_tick_null_context_is_invalid(crt):
    L = crt.lib()
    assert L.crt_tick(None, C.c_uint32(1), C.c_uint32(1), None, None, None) == -1     # CRT_ERR_INVALID


def test_header_declares_and_binding_wraps_crt_tick(crt):
    hdr = open(os.path.join(REPO, "include", "crt_abi.h")).read()
    assert "int  crt_tick(crt_ctx* ctx, uint32_t spp, uint32_t passes, uint32_t* host_pixels" in hdr
    assert "crt_tick" in crt.ABI_SYMBOLS
    getattr(crt.lib(), "crt_tick")
    assert callable(getattr(crt.Context, "tick", None))
