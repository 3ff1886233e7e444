"""Byte samples on ac_intg_dump (ACDSP_FLAG_IN_BYTES, IntgDump(in_bytes=True)): what acdsp_intgdump_create decides about a flagged descriptor
before it touches a device, and the pieces of the interface that carry the flag.  Runs with or without a GPU: a descriptor that passes
validation gets as far as the device check (ACDSP_ENODEVICE without one), a refused one fails with its code either way."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

import ac_dsp_amd as A
from ac_dsp_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _create(fin=A.Fmt(8, 4), **kw):
    kw.setdefault("in_bytes", True)
    return A.IntgDump(64, 4, fin, A.Fmt(32, 16), A.Fmt(32, 16), n_objects=2, **kw)


def test_a_flagged_descriptor_passes_validation():
    if torch.cuda.is_available():
        eng = _create()
        assert eng.in_bytes and eng.in_dtype == torch.int8 and L.lib.acdsp_intgdump_in_elem_bytes(eng._h) == 1
        eng.close()
        eng = _create(in_bytes=False)
        assert not eng.in_bytes and eng.in_dtype == torch.int16 and L.lib.acdsp_intgdump_in_elem_bytes(eng._h) == 2
        eng.close()
    else:
        with pytest.raises(A.AcdspError) as e:
            _create()
        assert e.value.code == 4, e.value             # ACDSP_ENODEVICE: validation passed, the device check did not


def test_an_unsigned_flagged_descriptor_passes_validation_through_the_raw_abi():
    d = L.IntgDumpDesc(16, 1, 1, A.Fmt(8, 8, False), A.Fmt(24, 24, False), A.Fmt(24, 24, False), 0, L.FLAG_IN_BYTES)
    h = C.c_void_p()
    rc = L.lib.acdsp_intgdump_create(C.byref(d), C.byref(h))
    if torch.cuda.is_available():
        assert rc == 0 and h.value
        assert L.lib.acdsp_intgdump_in_elem_bytes(h) == 1
        L.lib.acdsp_intgdump_destroy(h)
    else:
        assert rc == 4 and not h.value, rc


def test_the_flag_with_nine_bit_samples_is_invalid():
    with pytest.raises(A.AcdspError) as e:
        _create(fin=A.Fmt(9, 4))
    assert e.value.code == 1, e.value                 # ACDSP_EINVAL, with or without a device
    assert "W=9" in str(e.value) and "1-byte container" in str(e.value), e.value


def test_the_node_create_refuses_nine_bit_samples_too():
    d = L.IntgDumpDesc(64, 4, 2, A.Fmt(9, 4), A.Fmt(32, 16), A.Fmt(32, 16), 0, L.FLAG_IN_BYTES)
    h = C.c_void_p()
    devs = (C.c_int32 * 1)(0)
    rc = L.lib.acdsp_node_intgdump_create(C.byref(d), 1, devs, C.byref(h))
    assert rc != 0 and not h.value, rc
    if rc == 1:                                       # (without a device the node may stop at its own device check first)
        assert "W=9" in L.lib.acdsp_last_error().decode()


def test_in_elem_bytes_is_exported_declared_and_null_safe():
    assert L.lib.acdsp_intgdump_in_elem_bytes(None) == -1
    with open(os.path.join(ROOT, "include", "acdsp.h")) as f:
        hdr = f.read()
    assert re.search(r"int32_t\s+acdsp_intgdump_in_elem_bytes\(acdsp_intgdump_t h\);", hdr)
    assert "acdsp_intgdump_desc_t::flags" in hdr


def test_in_bytes_is_a_keyword_of_both_classes():
    for cls in (A.IntgDump, A.NodeIntgDump):
        p = inspect.signature(cls.__init__).parameters
        assert "in_bytes" in p and p["in_bytes"].default is False, cls
    assert callable(getattr(A.IntgDump, "run_host", None))
