"""Byte samples on the CIC decimator (ACDSP_FLAG_IN_BYTES, Cic(in_bytes=True)): what acdsp_cic_create, acdsp_ddc_create and
acdsp_node_ddc_create decide about a flagged descriptor before they touch a device, and the host-only acdsp_cic_two_stage_rates.  Runs with
or without a GPU: a descriptor that passes validation gets as far as the device check (ACDSP_ENODEVICE without one), a refused one fails with
its code either way."""
import ctypes as C

import pytest
import torch

import ac_dsp_amd as A
from ac_dsp_amd import _lib as L

F8 = A.Fmt(8, 1)
F16 = A.Fmt(16, 1)


def _create(R=64, M=1, N=4, fin=F8, fout=A.Fmt(32, 25), interp=False, **kw):
    kw.setdefault("in_bytes", True)
    return A.Cic(interp, R, M, N, fin, fout, **kw)


def test_a_flagged_decimator_passes_validation():
    if torch.cuda.is_available():
        cic = _create()
        assert cic.in_dtype == torch.int8 and L.lib.acdsp_cic_in_elem_bytes(cic._h) == 1
        cic.close()
    else:
        with pytest.raises(A.AcdspError) as e:
            _create()
        assert e.value.code == 4, e.value             # ACDSP_ENODEVICE: validation passed, the device check did not


def test_the_flag_with_nine_bit_samples_is_invalid():
    with pytest.raises(A.AcdspError) as e:
        _create(fin=A.Fmt(9, 1))
    assert e.value.code == 1, e.value                 # ACDSP_EINVAL
    assert "1-byte container" in str(e.value), e.value


def test_the_flag_on_an_interpolator_is_unsupported():
    with pytest.raises(A.AcdspError) as e:
        _create(R=8, N=3, interp=True)
    assert e.value.code == 2, e.value                 # ACDSP_EUNSUPPORTED
    assert "interp" in str(e.value), e.value


def test_the_flag_with_an_80_bit_output_type_is_unsupported():
    with pytest.raises(A.AcdspError) as e:
        _create(fout=A.Fmt(80, 60))
    assert e.value.code == 2, e.value
    assert "OUT_TYPE wider than 64 bits" in str(e.value), e.value


def _ddc_descs():
    it = A.Fmt(32, 25)
    cd = L.CicDesc(0, 16, 1, 5, 4, F8, A.Fmt(29, 22), 0, L.FLAG_IN_BYTES)
    fd = L.FirDesc(L.KINDS["const"], L.FTYPES["SHIFT_REG"], 63, 4, 0, A.Fmt(29, 22), A.Fmt(16, 1), A.Fmt(60, 30), it, 0, 0)
    return cd, fd


def test_a_flagged_decimator_in_a_ddc_cascade_is_unsupported():
    cd, fd = _ddc_descs()
    h = C.c_void_p()
    rc = L.lib.acdsp_ddc_create(C.byref(cd), C.byref(fd), C.byref(h))
    assert rc == 2 and not h.value, rc
    msg = L.lib.acdsp_last_error().decode()
    assert "ACDSP_FLAG_IN_BYTES" in msg and "CIC" in msg, msg


def test_a_flagged_decimator_in_a_node_ddc_cascade_is_unsupported():
    cd, fd = _ddc_descs()
    h = C.c_void_p()
    devs = (C.c_int32 * 1)(0)
    rc = L.lib.acdsp_node_ddc_create(C.byref(cd), C.byref(fd), 1, devs, C.byref(h))
    assert rc == 2 and not h.value, rc
    msg = L.lib.acdsp_last_error().decode()
    assert "ACDSP_FLAG_IN_BYTES" in msg and "CIC" in msg, msg


def _rates(fin, R, M, N, flags):
    it = A.Fmt()
    d = L.CicDesc(0, R, M, N, 1, fin, fin, 0, flags)
    L.check(L.lib.acdsp_cic_int_type(C.byref(d), C.byref(it)))
    d = L.CicDesc(0, R, M, N, 1, fin, A.Fmt(it.W, it.I), 0, flags)
    r1, r2 = C.c_int32(-1), C.c_int32(-1)
    L.check(L.lib.acdsp_cic_two_stage_rates(C.byref(d), C.byref(r1), C.byref(r2)))
    return r1.value, r2.value


@pytest.mark.parametrize("rmn,want", [((32, 1, 4), (16, 2)), ((24, 1, 4), (8, 3)), ((8, 1, 2), (4, 2)), ((244, 2, 3), (4, 61)),
                                      ((37, 1, 3), (0, 0)), ((6, 1, 3), (0, 0)), ((4, 1, 5), (0, 0))])
def test_two_stage_rates_of_flagged_descriptors(rmn, want):
    assert _rates(F8, *rmn, L.FLAG_IN_BYTES) == want


@pytest.mark.parametrize("rmn,want", [((64, 1, 4), (16, 4)), ((37, 1, 3), (0, 0))])
def test_two_stage_rates_of_unflagged_descriptors(rmn, want):
    assert _rates(F16, *rmn, 0) == want
