"""Byte samples on ac_poly_dec (ACDSP_FLAG_IN_BYTES, PolyDec(in_bytes=True)): what acdsp_polydec_create decides about a flagged descriptor
before it touches a device.  Runs with or without a GPU: a descriptor that passes validation gets as far as the device check
(ACDSP_ENODEVICE without one), a refused one fails with its code either way."""
import inspect

import pytest
import torch

import ac_dsp_amd as A

FIN = A.Fmt(8, 2)
FC = A.Fmt(16, 2)
FA = A.Fmt(40, 20)                          # F = 20 = F_in + F_coeff: exact products
FO = A.Fmt(16, 10, True, "RND", "SAT")


def _create(nt, df, fin=FIN, fa=FA, **kw):
    kw.setdefault("in_bytes", True)
    return A.PolyDec(nt, df, fin, FC, fa, FO, **kw)


@pytest.mark.parametrize("nt,df", [(16, 8), (256, 16)])      # NTAPS * DF = 128 (ring kernel) and 4096 (long byte kernel)
def test_a_byte_eligible_descriptor_passes_validation(nt, df):
    if torch.cuda.is_available():
        eng = _create(nt, df)
        assert eng.in_dtype == torch.int8 and eng.in_bytes
        assert A.lib.acdsp_polydec_in_elem_bytes(eng._h) == 1 and A.lib.acdsp_polydec_ring_shape(eng._h) == 0
        eng.close()
    else:
        with pytest.raises(A.AcdspError) as e:
            _create(nt, df)
        assert e.value.code == 4, e.value             # ACDSP_ENODEVICE: validation passed, the device check did not


@pytest.mark.parametrize("nt,df", [(16, 8), (256, 16)])
def test_the_flag_with_nine_bit_samples_is_invalid(nt, df):
    with pytest.raises(A.AcdspError) as e:
        _create(nt, df, fin=A.Fmt(9, 2))
    assert e.value.code == 1, e.value                 # ACDSP_EINVAL
    assert "IN_BYTES" in str(e.value), e.value


def test_flagged_with_a_lossy_accumulator_is_unsupported_at_4096_taps_and_names_the_condition():
    # (<40,20> keeps F = 20 and is exact; <40,22> keeps 18 and drops two bits of every product)
    with pytest.raises(A.AcdspError) as e:
        _create(256, 16, fa=A.Fmt(40, 22))
    assert e.value.code == 2, e.value                 # ACDSP_EUNSUPPORTED
    assert "exact-sum" in str(e.value), e.value


def test_the_in_bytes_keyword_exists_on_both_classes():
    for cls in (A.PolyDec, A.NodePolyDec):
        p = inspect.signature(cls.__init__).parameters
        assert "in_bytes" in p and p["in_bytes"].default is False, cls
    assert isinstance(A.PolyDec.in_dtype, property)


def test_the_new_symbols_are_exported():
    assert A.lib.acdsp_polydec_in_elem_bytes(None) == -1
    assert A.lib.acdsp_polydec_ring_shape(None) == -1
