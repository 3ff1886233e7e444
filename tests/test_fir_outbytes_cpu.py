"""Byte outputs (ACDSP_FLAG_OUT_BYTES, Fir(in_bytes=True, out_bytes=True)): what the create functions decide about the flag before they touch a
device.  Runs with or without a GPU: a descriptor that passes validation gets as far as the device check (ACDSP_ENODEVICE without one), a
refused one fails with its code either way."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

import ac_dsp_amd as A
from ac_dsp_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_BYTES = 4                               # ACDSP_FLAG_OUT_BYTES (spelled out: the attribute is part of what is tested)

FIN = A.Fmt(8, 2)
FC = A.Fmt(16, 2)
FA = A.Fmt(48, 28)                          # F = 20 = F_in + F_coeff: exact products
FO = A.Fmt(8, 8, True, "RND", "SAT")

EINVAL, EUNSUPPORTED, ENODEVICE = 1, 2, 4


def _fir_desc(flags, fo=FO, fin=FIN, n_taps=255):
    return L.FirDesc(L.KINDS["load"], L.FTYPES["SHIFT_REG"], n_taps, 2, 0, fin, FC, FA, fo, 0, flags)


def _create(fn, *descs):
    """(return code, message) of a raw create call; a handle that was created is destroyed again"""
    h = C.c_void_p()
    rc = fn(*[C.byref(d) for d in descs], C.byref(h))
    msg = L.lib.acdsp_last_error().decode() if rc else ""
    if rc == 0:
        getattr(L.lib, fn.__name__.replace("_create", "_destroy"))(h)
    return rc, msg


def _passed_validation(rc):
    return rc == (0 if torch.cuda.is_available() else ENODEVICE)


def test_the_flag_is_defined_on_both_sides():
    assert L.FLAG_OUT_BYTES == OUT_BYTES
    with open(os.path.join(ROOT, "include", "acdsp.h")) as f:
        hdr = f.read()
    assert re.search(r"#define\s+ACDSP_FLAG_OUT_BYTES\s+4\b", hdr)
    assert re.search(r"int32_t\s+acdsp_fir_out_elem_bytes\(acdsp_fir_t h\);", hdr)


def test_out_elem_bytes_is_exported_and_null_safe():
    assert L.lib.acdsp_fir_out_elem_bytes(None) == -1


def test_nine_bit_outputs_under_both_flags_are_invalid():
    rc, msg = _create(L.lib.acdsp_fir_create, _fir_desc(L.FLAG_IN_BYTES | OUT_BYTES, fo=A.Fmt(9, 8, True, "RND", "SAT")))
    assert rc == EINVAL, (rc, msg)
    assert "W=9" in msg and "1-byte container" in msg, msg
    with pytest.raises(A.AcdspError) as e:
        A.Fir(255, "SHIFT_REG", FIN, FC, FA, A.Fmt(9, 8, True, "RND", "SAT"), in_bytes=True, out_bytes=True)
    assert e.value.code == EINVAL, e.value


def test_the_output_flag_without_the_input_flag_is_unsupported():
    rc, msg = _create(L.lib.acdsp_fir_create, _fir_desc(OUT_BYTES))
    assert rc == EUNSUPPORTED, (rc, msg)
    assert "ACDSP_FLAG_IN_BYTES" in msg, msg
    rc, msg = _create(L.lib.acdsp_fir_create, _fir_desc(OUT_BYTES, fin=A.Fmt(16, 2)))
    assert rc == EUNSUPPORTED, (rc, msg)


@pytest.mark.parametrize("fo", [FO, A.Fmt(8, 8, False, "RND", "SAT"), A.Fmt(4, 7, True, "RND", "SAT"), A.Fmt(8, 8, False, "TRN", "WRAP")])
@pytest.mark.parametrize("n_taps", [255, 4097])
def test_a_valid_doubly_flagged_descriptor_reaches_the_device_check(fo, n_taps):
    rc, msg = _create(L.lib.acdsp_fir_create, _fir_desc(L.FLAG_IN_BYTES | L.FLAG_OUT_BYTES, fo=fo, n_taps=n_taps))
    assert _passed_validation(rc), (rc, msg)
    if torch.cuda.is_available():
        fir = A.Fir(n_taps, "SHIFT_REG", FIN, FC, FA, fo, n_channels=2, in_bytes=True, out_bytes=True)
        assert L.lib.acdsp_fir_out_elem_bytes(fir._h) == 1 and fir.out_dtype == (torch.int8 if fo.S else torch.uint8)
        twin = A.Fir(n_taps, "SHIFT_REG", FIN, FC, FA, fo, n_channels=2, in_bytes=True)
        assert L.lib.acdsp_fir_out_elem_bytes(twin._h) == 2 and twin.out_dtype == torch.int16


def _other_families(flags):
    f16, c16, a40 = A.Fmt(16, 2), A.Fmt(16, 2), A.Fmt(40, 12)
    return [
        ("cic", L.lib.acdsp_cic_create, (L.CicDesc(0, 8, 1, 5, 2, A.Fmt(32, 16), A.Fmt(47, 31), 0, flags),)),
        ("polydec", L.lib.acdsp_polydec_create, (L.PolyDecDesc(8, 4, 2, f16, c16, a40, A.Fmt(16, 2, True, "RND", "SAT"), 0, flags),)),
        ("polyintr", L.lib.acdsp_polyintr_create, (L.PolyIntrDesc(8, 40, 4, 0, 2, A.Fmt(32, 16), A.Fmt(32, 16), A.Fmt(64, 32), A.Fmt(64, 32), 0, flags),)),
        ("intgdump", L.lib.acdsp_intgdump_create, (L.IntgDumpDesc(64, 4, 2, A.Fmt(8, 4), A.Fmt(32, 16), A.Fmt(32, 16), 0, flags),)),
        ("mvavg", L.lib.acdsp_mvavg_create, (L.MvAvgDesc(64, 5, 0, 2, A.Fmt(16, 8), A.Fmt(16, 1), A.Fmt(32, 14), A.Fmt(32, 14), 0, flags),)),
    ]


@pytest.mark.parametrize("i", range(5))
def test_the_other_families_refuse_the_flag_instead_of_writing_int16_rows(i):
    name, fn, descs = _other_families(OUT_BYTES)[i]
    rc, msg = _create(fn, *descs)
    assert rc == EUNSUPPORTED, (name, rc, msg)
    assert "ACDSP_FLAG_OUT_BYTES" in msg, (name, msg)
    _, fn, descs = _other_families(0)[i]                 # the same descriptor without the flag is a valid one
    rc, msg = _create(fn, *descs)
    assert _passed_validation(rc), (name, rc, msg)


@pytest.mark.parametrize("stage", ["cic", "fir"])
def test_the_ddc_refuses_the_flag_on_either_stage(stage):
    # the cascade of the benchmark's DDC row: <16,2> samples, N = 4, R = 8 (INT_TYPE <28,14>), a 63-tap FIR behind it
    def descs(cic_flags, fir_flags):
        it = A.Fmt(28, 14)
        return (L.CicDesc(0, 8, 1, 4, 2, A.Fmt(16, 2), it, 0, cic_flags),
                L.FirDesc(L.KINDS["load"], L.FTYPES["SHIFT_REG"], 63, 2, 0, it, A.Fmt(16, 2), A.Fmt(48, 18), A.Fmt(32, 16), 0, fir_flags))
    rc, msg = _create(L.lib.acdsp_ddc_create, *descs(OUT_BYTES if stage == "cic" else 0, OUT_BYTES if stage == "fir" else 0))
    assert rc == EUNSUPPORTED, (rc, msg)
    assert "ACDSP_FLAG_OUT_BYTES" in msg, msg


def test_out_bytes_is_a_keyword_of_both_classes():
    for cls in (A.Fir, A.NodeFir):
        p = inspect.signature(cls.__init__).parameters
        assert "out_bytes" in p and p["out_bytes"].default is False, cls
        assert isinstance(getattr(cls, "out_dtype", None), property), cls
