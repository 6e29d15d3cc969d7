"""CPU: what every streaming handle's entries answer to a null handle, through the C ABI (no device call is made on these paths): put and
flush NAE_ERR_INVALID, available 0, receive NAE_ERR_INVALID, destroy NAE_OK; and the create entries that check their handle out-pointer
before any device call answer NAE_ERR_INVALID to a null one."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLES = ("stretch", "fir", "conv", "eq", "dyn", "spectrum", "wsola")


def status(name):
    """a code of enum nae_status, from include/nae_gpu.h"""
    m = re.search(r"\b%s\s*=\s*(-?\d+)" % name, open(os.path.join(ROOT, "include", "nae_gpu.h")).read())
    assert m, name
    return int(m.group(1))


OK, INVALID = status("NAE_OK"), status("NAE_ERR_INVALID")


def entries(lib, prefix, *names):
    """the entries of that handle the library has (the spectrum handle has no put_host, flush or receive_host)"""
    return [getattr(lib, f"nae_{prefix}_{n}") for n in names if hasattr(lib, f"nae_{prefix}_{n}")]


@pytest.mark.parametrize("prefix", HANDLES)
def test_null_handle(nae, prefix):
    lib = nae.load_library()
    one, got = (C.c_float * 2)(), C.c_size_t(77)
    puts = entries(lib, prefix, "put", "put_host")
    assert puts
    for put in puts:
        assert put(None, one, 1) == INVALID
        assert put(None, None, 0) == INVALID
    for flush in entries(lib, prefix, "flush"):
        assert flush(None) == INVALID
    assert getattr(lib, f"nae_{prefix}_available")(None) == 0
    receives = entries(lib, prefix, "receive", "receive_host")
    assert receives
    for receive in receives:
        assert receive(None, one, 1, C.byref(got)) == INVALID
        assert receive(None, None, 0, C.byref(got)) == INVALID
    assert getattr(lib, f"nae_{prefix}_destroy")(None) == OK


def test_create_with_a_null_handle_pointer(nae):
    """The entries that look at the out-pointer before they touch the context or the device."""
    lib = nae.load_library()
    taps, coef, params = (C.c_float * 3)(0, 1, 0), (C.c_double * 5)(1, 0, 0, 0, 0), nae.DynParams()
    assert lib.nae_stretch_create(None, 48000, 2, 1.0, 1.0, None) == INVALID
    assert lib.nae_stretch_create_ex(None, 48000, 2, 1.0, 1.0, 0, None) == INVALID
    assert lib.nae_stretch_create_n(None, 48000, 2, 1.0, 1.0, 0, 1024, None) == INVALID
    assert lib.nae_stretch_create_formant(None, 48000, 2, 1.0, 1.0, 0, 1024, 32, None) == INVALID
    assert lib.nae_stretch_create_formant_shift(None, 48000, 2, 1.0, 1.0, 0, 1024, 32, 1.25, None) == INVALID
    assert lib.nae_spectrum_create(None, 1024, 256, 2, None) == INVALID
    assert lib.nae_fir_create(None, taps, 3, 0, 2, None) == INVALID
    assert lib.nae_conv_create(None, taps, 3, 1, 0, 2, None) == INVALID
    assert lib.nae_eq_create(None, coef, 1, 2, None) == INVALID
    assert lib.nae_dyn_create(None, C.byref(params), 2, None) == INVALID
    assert lib.nae_wsola_create(None, 48000, 2, 1.0, 1.0, None) == INVALID
    assert lib.nae_swr_create(None, nae.FMT_FLT, 44100, 2, 48000, None) == INVALID
