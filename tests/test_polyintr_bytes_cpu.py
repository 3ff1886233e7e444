"""Byte rows on ac_poly_intr (ACDSP_FLAG_IN_BYTES / ACDSP_FLAG_OUT_BYTES, PolyIntr(in_bytes=True, out_bytes=True)): what acdsp_polyintr_create
decides about the flags before it touches a device, and the pieces of the interface that carry them.  Runs with or without a GPU: a descriptor
that passes validation gets as far as the device check (ACDSP_ENODEVICE without one), a refused one fails with its code either way."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

import ac_dsp_amd as A
from ac_dsp_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN_BYTES, OUT_BYTES = 2, 4                  # ACDSP_FLAG_IN_BYTES / ACDSP_FLAG_OUT_BYTES, spelled out
EINVAL, EUNSUPPORTED, ENODEVICE = 1, 2, 4
FOLD_EVEN, FOLD_ANTI = 0, 2

FIN = A.Fmt(8, 2)
FC = A.Fmt(16, 2)
FA = A.Fmt(32, 12)
FO = A.Fmt(8, 2, True, "RND", "SAT")


def _desc(flags, fin=FIN, fo=FO, fa=FA, n_taps=16, ifac=4, ftype=FOLD_EVEN, coeff_sz=None):
    return L.PolyIntrDesc(n_taps, coeff_sz or n_taps * ifac, ifac, ftype, 2, fin, FC, fa, fo, 0, flags)


def _create(desc):
    h = C.c_void_p()
    rc = L.lib.acdsp_polyintr_create(C.byref(desc), C.byref(h))
    msg = L.lib.acdsp_last_error().decode() if rc else ""
    if rc == 0:
        L.lib.acdsp_polyintr_destroy(h)
    return rc, msg


def _passed_validation(rc):
    return rc == (0 if torch.cuda.is_available() else ENODEVICE)


def test_nine_bit_samples_under_the_input_flag_are_invalid():
    rc, msg = _create(_desc(IN_BYTES, fin=A.Fmt(9, 2)))
    assert rc == EINVAL, (rc, msg)
    assert "W=9" in msg and "1-byte container" in msg and "IN_TYPE" in msg, msg
    with pytest.raises(A.AcdspError) as e:
        A.PolyIntr(16, 64, 4, "FOLD_EVEN", A.Fmt(9, 2), FC, FA, FO, in_bytes=True)
    assert e.value.code == EINVAL, e.value


@pytest.mark.parametrize("fo", [FO, A.Fmt(32, 14), A.Fmt(9, 4)])
def test_the_output_flag_alone_is_unsupported_whatever_the_output_type(fo):
    rc, msg = _create(_desc(OUT_BYTES, fo=fo))
    assert rc == EUNSUPPORTED, (rc, msg)
    assert "ACDSP_FLAG_OUT_BYTES" in msg and "ACDSP_FLAG_IN_BYTES" in msg, msg


def test_nine_bit_outputs_under_both_flags_are_invalid():
    rc, msg = _create(_desc(IN_BYTES | OUT_BYTES, fo=A.Fmt(9, 2, True, "RND", "SAT")))
    assert rc == EINVAL, (rc, msg)
    assert "W=9" in msg and "1-byte container" in msg and "OUT_TYPE" in msg, msg


def test_the_order_of_the_refusals():
    # nine-bit samples come first, whatever else is wrong; then the lone output flag; then nine-bit outputs
    wide_out = A.Fmt(9, 2, True, "RND", "SAT")
    rc, msg = _create(_desc(IN_BYTES | OUT_BYTES, fin=A.Fmt(9, 2), fo=wide_out))
    assert rc == EINVAL and "IN_TYPE" in msg and "W=9" in msg, (rc, msg)
    rc, msg = _create(_desc(OUT_BYTES, fin=A.Fmt(9, 2), fo=wide_out))
    assert rc == EUNSUPPORTED and "ACDSP_FLAG_IN_BYTES" in msg, (rc, msg)
    # ... and all of them in front of the family's own refusal of more than 2048 taps under the input flag
    rc, msg = _create(_desc(IN_BYTES | OUT_BYTES, fo=wide_out, n_taps=2049, ifac=2, ftype=FOLD_ANTI, fa=A.Fmt(40, 12)))
    assert rc == EINVAL and "OUT_TYPE" in msg, (rc, msg)


@pytest.mark.parametrize("flags", [IN_BYTES, IN_BYTES | OUT_BYTES])
@pytest.mark.parametrize("fin,fo", [(FIN, FO), (A.Fmt(8, 8, False), A.Fmt(8, 8, False, "TRN", "WRAP")), (A.Fmt(5, 2), A.Fmt(5, 1, True, "TRN", "WRAP")),
                                    (A.Fmt(5, 5, False), A.Fmt(4, 7, True, "RND", "SAT")), (A.Fmt(1, 1, False), A.Fmt(1, 1, True, "TRN", "SAT"))])
def test_valid_flagged_descriptors_reach_the_device_check(flags, fin, fo):
    rc, msg = _create(_desc(flags, fin=fin, fo=fo))
    assert _passed_validation(rc), (rc, msg)
    devs = (C.c_int32 * 1)(0)
    h = C.c_void_p()
    d = _desc(flags, fin=fin, fo=fo)
    rc = L.lib.acdsp_node_polyintr_create(C.byref(d), 1, devs, C.byref(h))
    if rc == 0:
        L.lib.acdsp_node_destroy(h)
    assert rc not in (EINVAL, EUNSUPPORTED), (rc, L.lib.acdsp_last_error().decode())
    assert torch.cuda.is_available() == (rc == 0), rc


def test_the_node_create_refuses_what_the_engine_refuses():
    devs = (C.c_int32 * 1)(0)
    for desc, code, word in ((_desc(IN_BYTES, fin=A.Fmt(9, 2)), EINVAL, "W=9"), (_desc(OUT_BYTES), EUNSUPPORTED, "ACDSP_FLAG_OUT_BYTES"),
                             (_desc(IN_BYTES | OUT_BYTES, fo=A.Fmt(9, 2)), EINVAL, "W=9")):
        h = C.c_void_p()
        rc = L.lib.acdsp_node_polyintr_create(C.byref(desc), 1, devs, C.byref(h))
        assert rc != 0 and not h.value, rc
        if rc == code:                                    # (without a device the node may stop at its own device check first)
            assert word in L.lib.acdsp_last_error().decode()


def test_more_than_2048_taps_under_the_input_flag_are_unsupported():
    # the long kernels read int16 rows: the same descriptor on 16-bit types, unflagged, is long-capable and passes
    kw = dict(n_taps=2049, ifac=2, ftype=FOLD_ANTI, fa=A.Fmt(40, 12))
    rc, msg = _create(_desc(IN_BYTES, fo=A.Fmt(16, 2, True, "RND", "SAT"), **kw))
    assert rc == EUNSUPPORTED, (rc, msg)
    assert "ACDSP_FLAG_IN_BYTES" in msg and "2048" in msg, msg
    rc, msg = _create(_desc(IN_BYTES | OUT_BYTES, **kw))
    assert rc == EUNSUPPORTED and "ACDSP_FLAG_IN_BYTES" in msg, (rc, msg)
    rc, msg = _create(_desc(0, fin=A.Fmt(16, 2), fo=A.Fmt(16, 2, True, "RND", "SAT"), **kw))
    assert _passed_validation(rc), (rc, msg)
    # 2048 taps stay: the exact kernels index rows by the container width
    rc, msg = _create(_desc(IN_BYTES | OUT_BYTES, n_taps=2048, ifac=2, ftype=FOLD_ANTI, fa=A.Fmt(40, 12)))
    assert _passed_validation(rc), (rc, msg)


def test_the_exports_exist_are_declared_and_null_safe():
    assert L.lib.acdsp_polyintr_in_elem_bytes(None) == -1
    assert L.lib.acdsp_polyintr_out_elem_bytes(None) == -1
    assert "acdsp_polyintr_in_elem_bytes" in L.SYMBOLS and "acdsp_polyintr_out_elem_bytes" in L.SYMBOLS
    with open(os.path.join(ROOT, "include", "acdsp.h")) as f:
        hdr = f.read()
    assert re.search(r"int32_t\s+acdsp_polyintr_in_elem_bytes\(acdsp_polyintr_t h\);", hdr)
    assert re.search(r"int32_t\s+acdsp_polyintr_out_elem_bytes\(acdsp_polyintr_t h\);", hdr)
    assert hdr.count("acdsp_polyintr_desc_t::flags") >= 2      # named under both flags


def test_the_keywords_and_dtype_properties_of_both_classes():
    for cls in (A.PolyIntr, A.NodePolyIntr):
        p = inspect.signature(cls.__init__).parameters
        for kw in ("in_bytes", "out_bytes"):
            assert kw in p and p[kw].default is False, (cls, kw)
        for prop in ("in_dtype", "out_dtype"):
            assert isinstance(getattr(cls, prop, None), property), (cls, prop)
    assert callable(getattr(A.PolyIntr, "run_host", None))


@pytest.mark.parametrize("in_bytes,out_bytes,want", [(True, True, (1, 1)), (True, False, (1, 2)), (False, False, (2, 2))])
def test_the_container_widths_of_a_handle(in_bytes, out_bytes, want):
    """with a GPU: what a live handle reports; without one the constructor stops at the device check"""
    if not torch.cuda.is_available():
        with pytest.raises(A.AcdspError) as e:
            A.PolyIntr(16, 64, 4, "FOLD_EVEN", FIN, FC, A.Fmt(40, 12), FO, n_channels=2, in_bytes=in_bytes, out_bytes=out_bytes)
        assert e.value.code == ENODEVICE, e.value
        return
    for fin, fo in ((FIN, FO), (A.Fmt(8, 8, False), A.Fmt(8, 8, False, "TRN", "WRAP"))):
        e = A.PolyIntr(16, 64, 4, "FOLD_EVEN", fin, FC, A.Fmt(40, 12), fo, n_channels=2, in_bytes=in_bytes, out_bytes=out_bytes)
        assert (L.lib.acdsp_polyintr_in_elem_bytes(e._h), L.lib.acdsp_polyintr_out_elem_bytes(e._h)) == want
        assert e.in_dtype == ((torch.int8 if fin.S else torch.uint8) if in_bytes else torch.int16)
        assert e.out_dtype == ((torch.int8 if fo.S else torch.uint8) if out_bytes else torch.int16)
