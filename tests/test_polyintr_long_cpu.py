"""Long ac_poly_intr sub-filters (NTAPS + lag = 65 .. 16384 taps per phase): what acdsp_polyintr_create decides about a descriptor before it
touches a device.  Runs with or without a GPU: an eligible descriptor gets as far as the device check (ACDSP_ENODEVICE without one), an
ineligible one above 2048 taps is ACDSP_EUNSUPPORTED either way, and up to 2048 taps nothing new is refused."""
import pytest
import torch

import ac_dsp_amd as A

FIN = FC = A.Fmt(16, 2)
FA = A.Fmt(48, 20)
FO = A.Fmt(16, 10, True, "RND", "SAT")


def table_size(n_taps, ifac, ftype):
    j = ifac - 1
    return {"FOLD_EVEN": (n_taps // 2 - 1) + j * n_taps // 2, "FOLD_ODD": (n_taps - 1) // 2 + (n_taps // 2 + 1) * j,
            "FOLD_ANTI": (n_taps - 1) + n_taps * j}[ftype] + 1


def _create(n_taps=4096, ifac=4, ftype="FOLD_EVEN", fin=FIN, fc=FC, fa=FA, fo=FO, **kw):
    return A.PolyIntr(n_taps, table_size(n_taps, ifac, ftype), ifac, ftype, fin, fc, fa, fo, **kw)


def _reaches_the_device_check(**kw):
    if torch.cuda.is_available():
        _create(**kw).close()
    else:
        with pytest.raises(A.AcdspError) as e:
            _create(**kw)
        assert e.value.code == 4, (kw, e.value)   # ACDSP_ENODEVICE: validation passed, the device check did not


def test_an_eligible_4096_x_4_descriptor_passes_validation():
    _reaches_the_device_check()


@pytest.mark.parametrize("kw", [
    dict(n_taps=16383, ifac=1, ftype="FOLD_ODD"),     # nt = 16384
    dict(n_taps=16384, ifac=1, ftype="FOLD_ANTI"),
    dict(n_taps=8192, ifac=2),
])
def test_the_largest_prototypes_pass_validation(kw):
    _reaches_the_device_check(**kw)


@pytest.mark.parametrize("what,names,kw", [
    ("32-bit samples", "IN_TYPE", dict(fin=A.Fmt(32, 16))),
    # (<40,12> keeps F = 28 = F_in + F_coeff bits and is exact; <40,14> keeps 26 and drops two bits of every product)
    ("a lossy accumulator", "ACC_TYPE", dict(fa=A.Fmt(40, 14))),
    ("a saturating accumulator", "ACC_TYPE", dict(fa=A.Fmt(48, 20, True, "TRN", "SAT"))),
    ("an 80-bit accumulator", "ACC_TYPE", dict(fa=A.Fmt(80, 30))),
    ("force_generic above 2048 taps", "FORCE_GENERIC", dict(force_generic=True)),
    ("NTAPS 16384 on a folded core (nt = 16385)", "outside 1..16383", dict(n_taps=16384, ifac=1)),
    ("4096 x 16: 16 x 129 K-blocks", "K-block budget", dict(ifac=16)),
])
def test_ineligible_long_descriptors_are_unsupported_with_or_without_a_device(what, names, kw):
    with pytest.raises(A.AcdspError) as e:
        _create(**kw)
    assert e.value.code == 2, (what, e.value)   # ACDSP_EUNSUPPORTED
    assert names in str(e.value), (what, e.value)   # the refusal names the failed condition


@pytest.mark.parametrize("kw", [
    dict(n_taps=2048, fin=A.Fmt(32, 16), fc=A.Fmt(32, 16), fa=A.Fmt(64, 32), fo=A.Fmt(32, 16)),
    dict(n_taps=2048, fa=A.Fmt(40, 14)),
    dict(n_taps=2048, fa=A.Fmt(48, 20, True, "TRN", "SAT")),
    dict(n_taps=2048, force_generic=True),
    dict(n_taps=2048, ifac=16),                       # 16 x 65 K-blocks: over the budget, keeps its old kernel
    dict(n_taps=100, ifac=255, ftype="FOLD_ANTI", fin=A.Fmt(32, 16)),
])
def test_shapes_of_up_to_2048_taps_are_validated_as_before(kw):
    # none of the long-only conditions refuses a shape of 2048 taps or fewer: these get as far as the device check
    _reaches_the_device_check(**kw)
