"""Long ac_poly_dec prototypes (NTAPS*DF up to 16384, DF up to 256): what acdsp_polydec_create decides about a descriptor before it touches a
device.  Runs with or without a GPU: an eligible descriptor gets as far as the device check (ACDSP_ENODEVICE without one), an ineligible one
above 2048 taps is ACDSP_EUNSUPPORTED either way, and up to 2048 taps nothing new is refused."""
import pytest
import torch

import ac_dsp_amd as A

FIN = FC = A.Fmt(16, 2)
FA = A.Fmt(48, 20)
FO = A.Fmt(16, 10, True, "RND", "SAT")


def _create(n_taps=256, df=16, fin=FIN, fc=FC, fa=FA, fo=FO, **kw):
    return A.PolyDec(n_taps, df, fin, fc, fa, fo, **kw)


def _reaches_the_device_check(**kw):
    if torch.cuda.is_available():
        _create(**kw).close()
    else:
        with pytest.raises(A.AcdspError) as e:
            _create(**kw)
        assert e.value.code == 4, (kw, e.value)   # ACDSP_ENODEVICE: validation passed, the device check did not


def test_an_eligible_256_x_16_descriptor_passes_validation():
    _reaches_the_device_check()


@pytest.mark.parametrize("what,names,kw", [
    ("NTAPS*DF = 16400", "outside 1..16384", dict(n_taps=1025, df=16)),
    ("16 x 257", "DF outside", dict(n_taps=16, df=257)),
    ("32-bit samples", "IN_TYPE", dict(fin=A.Fmt(32, 16))),
    # (<40,12> keeps F = 28 = F_in + F_coeff bits and is exact; <40,14> keeps 26 and drops two bits of every product)
    ("a lossy accumulator", "ACC_TYPE", dict(fa=A.Fmt(40, 14))),
    ("an 80-bit accumulator", "ACC_TYPE", dict(fa=A.Fmt(80, 30))),
    ("force_generic above 2048 taps", "FORCE_GENERIC", dict(force_generic=True)),
])
def test_ineligible_long_descriptors_are_unsupported_with_or_without_a_device(what, names, kw):
    with pytest.raises(A.AcdspError) as e:
        _create(**kw)
    assert e.value.code == 2, (what, e.value)   # ACDSP_EUNSUPPORTED
    assert names in str(e.value), (what, e.value)   # the refusal names the failed condition


@pytest.mark.parametrize("kw", [
    dict(n_taps=8, df=256, fin=A.Fmt(32, 16), fc=A.Fmt(32, 16), fa=A.Fmt(64, 32), fo=A.Fmt(32, 16)),
    dict(n_taps=4, df=257),
])
def test_shapes_of_up_to_2048_taps_are_validated_as_before(kw):
    # none of the long-only conditions refuses a shape of 2048 taps or fewer: these get as far as the device check
    _reaches_the_device_check(**kw)
