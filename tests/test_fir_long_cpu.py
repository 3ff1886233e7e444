"""Long FIRs (1026 .. 16384 taps): what acdsp_fir_create decides about a descriptor before it touches a device.  Runs with or without a GPU:
an eligible descriptor gets as far as the device check (ACDSP_ENODEVICE without one), an ineligible one is ACDSP_EUNSUPPORTED either way."""
import pytest
import torch

import ac_dsp_amd as A

FIN = FC = A.Fmt(16, 2)
FA = A.Fmt(48, 20)
FO = A.Fmt(16, 10, True, "RND", "SAT")


def _create(n_taps=4096, ftype="SHIFT_REG", fin=FIN, fc=FC, fa=FA, fo=FO, **kw):
    kw.setdefault("kind", "load")
    return A.Fir(n_taps, ftype, fin, fc, fa, fo, **kw)


def test_an_eligible_4096_tap_descriptor_passes_validation():
    if torch.cuda.is_available():
        fir = _create()
        assert fir.n_taps == 4096
        fir.close()
    else:
        with pytest.raises(A.AcdspError) as e:
            _create()
        assert e.value.code == 4, e.value   # ACDSP_ENODEVICE: validation passed, the device check did not


@pytest.mark.parametrize("what,kw", [
    ("more than 16384 taps", dict(n_taps=16385)),
    ("a coefficient set per channel", dict(n_channels=2, coeffs_per_channel=True)),
    ("32-bit samples", dict(fin=A.Fmt(32, 16))),
    # (<40,12> keeps F = 28 = F_in + F_coeff bits and is exact; <40,14> keeps 26 and drops two bits of every product)
    ("a lossy accumulator", dict(fa=A.Fmt(40, 14))),
    ("an 80-bit accumulator", dict(fa=A.Fmt(80, 30))),
    ("TRANSPOSED with loadable coefficients", dict(ftype="TRANSPOSED")),
    ("force_generic", dict(force_generic=True)),
])
def test_ineligible_long_descriptors_are_unsupported_with_or_without_a_device(what, kw):
    with pytest.raises(A.AcdspError) as e:
        _create(**kw)
    assert e.value.code == 2, (what, e.value)   # ACDSP_EUNSUPPORTED


def test_the_refusal_names_the_failed_condition():
    with pytest.raises(A.AcdspError) as e:
        _create(fin=A.Fmt(32, 16))
    assert "IN_TYPE" in str(e.value), e.value
    with pytest.raises(A.AcdspError) as e:
        _create(ftype="TRANSPOSED")
    assert "TRANSPOSED" in str(e.value), e.value


def test_descriptors_up_to_2048_taps_are_validated_as_before():
    # none of the long-only conditions applies at 2048 taps and below: these get as far as the device check
    for kw in (dict(n_taps=2048, force_generic=True), dict(n_taps=2048, fin=A.Fmt(32, 16), fa=A.Fmt(64, 32)), dict(n_taps=1026, ftype="TRANSPOSED")):
        if torch.cuda.is_available():
            _create(**kw).close()
        else:
            with pytest.raises(A.AcdspError) as e:
                _create(**kw)
            assert e.value.code == 4, (kw, e.value)
