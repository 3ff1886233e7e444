"""Byte samples on the DDC cascade (ACDSP_DDC_IN_BYTES, Ddc(in_bytes=True)): what acdsp_ddc_create_ex and acdsp_node_ddc_create_ex decide
about the cascade's flags and its stage descriptors before they touch a device.  The container flag belongs to the composite: a byte flag on
a stage descriptor stays refused as under acdsp_ddc_create.  Runs with or without a GPU: a descriptor pair that passes validation gets as far
as the device check (ACDSP_ENODEVICE without one), a refused one fails with its code either way."""
import ctypes as C

import pytest
import torch

import ac_dsp_amd as A
from ac_dsp_amd import _lib as L

EINVAL, EUNSUPPORTED, ENODEVICE = 1, 2, 4
F8, U8 = A.Fmt(8, 1), A.Fmt(8, 8, False)


def _descs(fin=F8, cic_flags=0, fir_flags=0, R=16, N=5, n_ch=4, mid=None):
    if mid is None:
        it = A.Fmt()
        L.check(L.lib.acdsp_cic_int_type(C.byref(L.CicDesc(0, R, 1, N, n_ch, fin, fin, 0, 0)), C.byref(it)))
        mid = A.Fmt(it.W, it.I)
    cd = L.CicDesc(0, R, 1, N, n_ch, fin, mid, 0, cic_flags)
    fd = L.FirDesc(L.KINDS["const"], L.FTYPES["SHIFT_REG"], 127, n_ch, 0, mid, A.Fmt(16, 1), A.Fmt(60, 30), A.Fmt(24, 9, True, "RND", "SAT"), 0, fir_flags)
    return cd, fd


def _engine(cd, fd, ddc_flags):
    h = C.c_void_p()
    rc = L.lib.acdsp_ddc_create_ex(C.byref(cd), C.byref(fd), ddc_flags, C.byref(h))
    msg = L.lib.acdsp_last_error().decode()
    if h.value:
        L.lib.acdsp_ddc_destroy(h)
    return rc, msg


def _node(cd, fd, ddc_flags):
    h = C.c_void_p()
    devs = (C.c_int32 * 1)(0)
    rc = L.lib.acdsp_node_ddc_create_ex(C.byref(cd), C.byref(fd), ddc_flags, 1, devs, C.byref(h))
    msg = L.lib.acdsp_last_error().decode()
    if h.value:
        L.lib.acdsp_node_destroy(h)
    return rc, msg


CREATE = pytest.mark.parametrize("create", [_engine, _node], ids=["engine", "node"])
PASSED = 0 if torch.cuda.is_available() else ENODEVICE   # validation passed: the handle exists, or only the device check failed


@CREATE
@pytest.mark.parametrize("fin", [F8, U8], ids=["s8", "u8"])
def test_a_valid_byte_cascade_passes_validation(create, fin):
    rc, msg = create(*_descs(fin), L.DDC_IN_BYTES)
    assert rc == PASSED, (rc, msg)


def test_the_python_classes_take_the_option():
    for fin, dt in ((F8, torch.int8), (U8, torch.uint8)):
        if torch.cuda.is_available():
            d = A.Ddc(16, 1, 5, fin, 127, "SHIFT_REG", A.Fmt(16, 1), A.Fmt(60, 30), A.Fmt(24, 9, True, "RND", "SAT"), n_channels=2, in_bytes=True)
            assert d.in_dtype == dt and L.lib.acdsp_ddc_in_elem_bytes(d._h) == 1
            d.close()
        else:
            with pytest.raises(A.AcdspError) as e:
                A.Ddc(16, 1, 5, fin, 127, "SHIFT_REG", A.Fmt(16, 1), A.Fmt(60, 30), A.Fmt(24, 9, True, "RND", "SAT"), n_channels=2, in_bytes=True)
            assert e.value.code == ENODEVICE, e.value
            with pytest.raises(A.AcdspError) as e:
                A.NodeDdc(16, 1, 5, fin, 127, "SHIFT_REG", A.Fmt(16, 1), A.Fmt(60, 30), A.Fmt(24, 9, True, "RND", "SAT"), 2, [0], in_bytes=True)
            assert e.value.code == ENODEVICE, e.value
    assert L.lib.acdsp_ddc_in_elem_bytes(None) == -1


@CREATE
def test_the_flag_with_nine_bit_samples_is_invalid(create):
    rc, msg = create(*_descs(A.Fmt(9, 1)), L.DDC_IN_BYTES)
    assert rc == EINVAL, (rc, msg)
    assert "1-byte container" in msg, msg


@CREATE
def test_an_unknown_cascade_flag_is_invalid(create):
    for flags in (2, 4, L.DDC_IN_BYTES | 8, -2):
        rc, msg = create(*_descs(), flags)
        assert rc == EINVAL, (flags, rc, msg)
        assert "ddc_flags" in msg, msg


@CREATE
@pytest.mark.parametrize("ddc_flags", [0, L.DDC_IN_BYTES])
def test_byte_flags_on_a_stage_descriptor_stay_refused(create, ddc_flags):
    rc, msg = create(*_descs(cic_flags=L.FLAG_IN_BYTES), ddc_flags)
    assert rc == EUNSUPPORTED and "ACDSP_FLAG_IN_BYTES" in msg and "CIC" in msg, (rc, msg)
    rc, msg = create(*_descs(fir_flags=L.FLAG_IN_BYTES), ddc_flags)
    assert rc == EUNSUPPORTED and "ACDSP_FLAG_IN_BYTES" in msg and "FIR" in msg, (rc, msg)
    for where in ("cic_flags", "fir_flags"):
        rc, msg = create(*_descs(**{where: L.FLAG_OUT_BYTES}), ddc_flags)
        assert rc == EUNSUPPORTED and "ACDSP_FLAG_OUT_BYTES" in msg, (where, rc, msg)


def test_the_stage_flags_are_refused_before_the_sample_width():
    # both wrong: the stage-flag refusal comes first (the order of include/acdsp.h)
    rc, msg = _engine(*_descs(A.Fmt(9, 1), cic_flags=L.FLAG_IN_BYTES), L.DDC_IN_BYTES)
    assert rc == EUNSUPPORTED, (rc, msg)
    rc, msg = _engine(*_descs(A.Fmt(9, 1)), L.DDC_IN_BYTES | 2)
    assert rc == EINVAL and "ddc_flags" in msg, (rc, msg)


def test_flags_zero_is_acdsp_ddc_create():
    def plain(cd, fd):
        h = C.c_void_p()
        rc = L.lib.acdsp_ddc_create(C.byref(cd), C.byref(fd), C.byref(h))
        msg = L.lib.acdsp_last_error().decode()
        if h.value:
            L.lib.acdsp_ddc_destroy(h)
        return rc, msg

    good = _descs(A.Fmt(16, 1))
    assert plain(*good)[0] == _engine(*good, 0)[0] == PASSED
    bad = _descs(A.Fmt(16, 1), mid=A.Fmt(30, 15))            # a decimator output narrower than its INT_TYPE <36,21>
    r0, r1 = plain(*bad), _engine(*bad, 0)
    if torch.cuda.is_available():
        assert r0 == r1 and r0[0] == EINVAL and "INT_TYPE" in r0[1], (r0, r1)
    else:
        assert r0 == r1 and r0[0] == ENODEVICE, (r0, r1)         # (that check needs the stage handles: it stands behind the device check)
    bad2 = _descs(A.Fmt(16, 1))
    bad2[1].n_channels = 3                                     # the stages disagree about the channel count
    r0, r1 = plain(*bad2), _engine(*bad2, 0)
    assert r0 == r1 and r0[0] == EINVAL and "same channels" in r0[1], (r0, r1)
