"""Byte samples (ACDSP_FLAG_IN_BYTES, Fir(in_bytes=True)): what acdsp_fir_create decides about a flagged descriptor before it touches a device.
Runs with or without a GPU: a descriptor that passes validation gets as far as the device check (ACDSP_ENODEVICE without one), a refused one
fails with its code either way."""
import pytest
import torch

import ac_dsp_amd as A

FIN = A.Fmt(8, 2)
FC = A.Fmt(16, 2)
FA = A.Fmt(48, 28)                          # F = 20 = F_in + F_coeff: exact products
FO = A.Fmt(16, 10, True, "RND", "SAT")

# the four ways a flagged descriptor misses the byte-sample kernel, with a word of the condition the refusal must name
NOT_ELIGIBLE = [
    ("a coefficient set per channel", dict(n_channels=2, coeffs_per_channel=True), "per channel"),
    # (<40,20> keeps F = 20 and is exact; <40,22> keeps 18 and drops two bits of every product)
    ("a lossy accumulator", dict(fa=A.Fmt(40, 22)), "exact-sum"),
    ("TRANSPOSED with loadable coefficients", dict(ftype="TRANSPOSED"), "TRANSPOSED"),
    ("force_generic", dict(force_generic=True), "FORCE_GENERIC"),
]


def _create(n_taps=4096, ftype="SHIFT_REG", fin=FIN, fc=FC, fa=FA, fo=FO, **kw):
    kw.setdefault("kind", "load")
    kw.setdefault("in_bytes", True)
    return A.Fir(n_taps, ftype, fin, fc, fa, fo, **kw)


def _passes_validation(**kw):
    if torch.cuda.is_available():
        fir = _create(**kw)
        assert fir.in_dtype == torch.int8
        fir.close()
    else:
        with pytest.raises(A.AcdspError) as e:
            _create(**kw)
        assert e.value.code == 4, (kw, e.value)   # ACDSP_ENODEVICE: validation passed, the device check did not


@pytest.mark.parametrize("n_taps", [255, 4096])
def test_a_byte_eligible_descriptor_passes_validation(n_taps):
    _passes_validation(n_taps=n_taps)


def test_the_flag_with_nine_bit_samples_is_invalid():
    with pytest.raises(A.AcdspError) as e:
        _create(n_taps=255, fin=A.Fmt(9, 2))
    assert e.value.code == 1, e.value             # ACDSP_EINVAL


def test_the_flag_with_an_80_bit_accumulator_is_unsupported():
    with pytest.raises(A.AcdspError) as e:
        _create(n_taps=255, fa=A.Fmt(80, 60))
    assert e.value.code == 2, e.value             # ACDSP_EUNSUPPORTED


@pytest.mark.parametrize("what,kw,word", NOT_ELIGIBLE)
def test_flagged_and_not_eligible_is_unsupported_at_4096_taps_and_names_the_condition(what, kw, word):
    with pytest.raises(A.AcdspError) as e:
        _create(n_taps=4096, **kw)
    assert e.value.code == 2, (what, e.value)
    assert word in str(e.value), (what, e.value)


@pytest.mark.parametrize("what,kw,word", NOT_ELIGIBLE)
def test_the_same_descriptors_pass_validation_at_2048_taps(what, kw, word):
    _passes_validation(n_taps=2048, **kw)
