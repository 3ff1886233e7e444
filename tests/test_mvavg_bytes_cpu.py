"""Byte rows on ac_mv_avg (ACDSP_FLAG_IN_BYTES / ACDSP_FLAG_OUT_BYTES, MvAvg(in_bytes=True, out_bytes=True)): what acdsp_mvavg_create decides
about the flags before it touches a device, the pieces of the interface that carry them, and the Toeplitz fragments of the byte-plane kernel
(host only).  Runs with or without a GPU: a descriptor that passes validation gets as far as the device check (ACDSP_ENODEVICE without one), a
refused one fails with its code either way."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import ac_dsp_amd as A
from ac_dsp_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN_BYTES, OUT_BYTES = 2, 4                  # ACDSP_FLAG_IN_BYTES / ACDSP_FLAG_OUT_BYTES, spelled out
EINVAL, EUNSUPPORTED, ENODEVICE = 1, 2, 4

FIN = A.Fmt(8, 4)
FC = A.Fmt(16, 1)
FA = A.Fmt(32, 10)
FO = A.Fmt(8, 4, True, "RND", "SAT")


def _desc(flags, fin=FIN, fo=FO):
    return L.MvAvgDesc(64, 5, 0, 2, fin, FC, FA, fo, 0, flags)


def _create(desc):
    h = C.c_void_p()
    rc = L.lib.acdsp_mvavg_create(C.byref(desc), C.byref(h))
    msg = L.lib.acdsp_last_error().decode() if rc else ""
    if rc == 0:
        L.lib.acdsp_mvavg_destroy(h)
    return rc, msg


def _passed_validation(rc):
    return rc == (0 if torch.cuda.is_available() else ENODEVICE)


def test_nine_bit_samples_under_the_input_flag_are_invalid():
    rc, msg = _create(_desc(IN_BYTES, fin=A.Fmt(9, 4)))
    assert rc == EINVAL, (rc, msg)
    assert "W=9" in msg and "1-byte container" in msg, msg
    with pytest.raises(A.AcdspError) as e:
        A.MvAvg(64, 5, "WIN", A.Fmt(9, 4), FC, FA, FO, in_bytes=True)
    assert e.value.code == EINVAL, e.value


@pytest.mark.parametrize("fo", [FO, A.Fmt(32, 14), A.Fmt(9, 4)])
def test_the_output_flag_alone_is_unsupported_whatever_the_output_type(fo):
    rc, msg = _create(_desc(OUT_BYTES, fo=fo))
    assert rc == EUNSUPPORTED, (rc, msg)
    assert "ACDSP_FLAG_OUT_BYTES" in msg and "ACDSP_FLAG_IN_BYTES" in msg, msg


def test_nine_bit_outputs_under_both_flags_are_invalid():
    rc, msg = _create(_desc(IN_BYTES | OUT_BYTES, fo=A.Fmt(9, 4, True, "RND", "SAT")))
    assert rc == EINVAL, (rc, msg)
    assert "W=9" in msg and "1-byte container" in msg and "OUT_TYPE" in msg, msg


@pytest.mark.parametrize("flags", [IN_BYTES, IN_BYTES | OUT_BYTES])
@pytest.mark.parametrize("fin,fo", [(FIN, FO), (A.Fmt(8, 8, False), A.Fmt(8, 8, False, "TRN", "WRAP")), (A.Fmt(5, 5, False), A.Fmt(4, 7, True, "RND", "SAT")),
                                    (A.Fmt(1, 1, False), A.Fmt(3, 3, False, "TRN", "SAT"))])
def test_valid_flagged_descriptors_reach_the_device_check(flags, fin, fo):
    rc, msg = _create(_desc(flags, fin=fin, fo=fo))
    assert _passed_validation(rc), (rc, msg)
    if torch.cuda.is_available():
        m = A.MvAvg(64, 5, "WIN", fin, FC, FA, fo, n_objects=2, in_bytes=True, out_bytes=bool(flags & OUT_BYTES))
        assert L.lib.acdsp_mvavg_in_elem_bytes(m._h) == 1 and m.in_dtype == (torch.int8 if fin.S else torch.uint8)
        assert L.lib.acdsp_mvavg_out_elem_bytes(m._h) == (1 if flags & OUT_BYTES else 2)
        assert m.out_dtype == ((torch.int8 if fo.S else torch.uint8) if flags & OUT_BYTES else torch.int16)
        twin = A.MvAvg(64, 5, "WIN", fin, FC, FA, fo, n_objects=2)
        assert L.lib.acdsp_mvavg_in_elem_bytes(twin._h) == 2 and twin.in_dtype == torch.int16 and twin.out_dtype == torch.int16


def test_the_node_create_refuses_what_the_engine_refuses():
    devs = (C.c_int32 * 1)(0)
    for desc, code, word in ((_desc(IN_BYTES, fin=A.Fmt(9, 4)), EINVAL, "W=9"), (_desc(OUT_BYTES), EUNSUPPORTED, "ACDSP_FLAG_OUT_BYTES")):
        h = C.c_void_p()
        rc = L.lib.acdsp_node_mvavg_create(C.byref(desc), 1, devs, C.byref(h))
        assert rc != 0 and not h.value, rc
        if rc == code:                                    # (without a device the node may stop at its own device check first)
            assert word in L.lib.acdsp_last_error().decode()


def test_the_exports_exist_are_declared_and_null_safe():
    assert L.lib.acdsp_mvavg_in_elem_bytes(None) == -1
    assert L.lib.acdsp_mvavg_out_elem_bytes(None) == -1
    with open(os.path.join(ROOT, "include", "acdsp.h")) as f:
        hdr = f.read()
    assert re.search(r"int32_t\s+acdsp_mvavg_in_elem_bytes\(acdsp_mvavg_t h\);", hdr)
    assert re.search(r"int32_t\s+acdsp_mvavg_out_elem_bytes\(acdsp_mvavg_t h\);", hdr)
    assert hdr.count("acdsp_mvavg_desc_t::flags") >= 2      # named under both flags


def test_the_keywords_and_dtype_properties_of_both_classes():
    for cls in (A.MvAvg, A.NodeMvAvg):
        p = inspect.signature(cls.__init__).parameters
        for kw in ("in_bytes", "out_bytes"):
            assert kw in p and p[kw].default is False, (cls, kw)
        for prop in ("in_dtype", "out_dtype"):
            assert isinstance(getattr(cls, prop, None), property), (cls, prop)
    assert callable(getattr(A.MvAvg, "run_host", None))


# ---- the fragment builder in the byte geometry (acdsp_mvavg_frags_host: no device) ----------------------------------------------------------
FRAG_WORDS = 2048                           # ACDSP_MVAVG_FRAG_WORDS
SPECIAL = [127, -128, 128, 255, -129, 32639]


def _frags(c, taps, mode, in_bytes=1):
    c = np.ascontiguousarray(c, dtype=np.int64)
    out = np.zeros(FRAG_WORDS, dtype=np.uint32)
    csum, hi = C.c_int64(), C.c_int32()
    nb = L.lib.acdsp_mvavg_frags_host(c.ctypes.data_as(C.POINTER(C.c_int64)), taps, mode, in_bytes, out.ctypes.data_as(C.POINTER(C.c_uint32)),
                                      C.byref(csum), C.byref(hi))
    return nb, out, csum.value, hi.value


def _toeplitz_from_frags(frags, nb, img):
    """What mv_avg_s8_kernel computes for one 512-output tile from the byte image `img` (signed samples): lane (j' = lane & 15, kg = lane >> 4)
    multiplies A[i][16 kg .. 16 kg + 15] of K block b with image bytes 32 j' + 64 b + 16 kg ..; row i of row order m of column j' is output
    32 j' + 8 (i >> 2) + (i & 3) + 4 m; the two digit planes weigh 1 and 256."""
    fr = frags[:2 * nb * 2 * 64 * 4].view(np.int8).astype(np.int64).reshape(2, nb, 2, 64, 16)   # [m][b][plane][lane][16 bytes]
    out = np.zeros(512, dtype=np.int64)
    for m in range(2):
        for b in range(nb):
            dig = fr[m, b, 0] + 256 * fr[m, b, 1]                          # [lane][16]
            A_ = np.zeros((16, 64), dtype=np.int64)                        # A[i][kk]
            for lane in range(64):
                A_[lane & 15, 16 * (lane >> 4):16 * (lane >> 4) + 16] = dig[lane]
            for j in range(16):
                col = img[32 * j + 64 * b:32 * j + 64 * b + 64]
                prod = A_ @ col
                for i in range(16):
                    out[32 * j + 8 * (i >> 2) + (i & 3) + 4 * m] += prod[i]
    return out


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_the_fragments_of_the_byte_geometry_form_the_window_sums(mode):
    rng = np.random.default_rng(20 + mode)
    for taps in range(1, 66, 2):
        c = rng.integers(-300, 300, taps)
        pos = rng.permutation(taps)[:len(SPECIAL)]
        for p_, v in zip(pos, SPECIAL):
            c[p_] = v
        if taps < len(SPECIAL):                                            # short windows: the specials take turns
            c[:] = [SPECIAL[(taps + k) % len(SPECIAL)] for k in range(taps)]
        nb, frags, csum, hi = _frags(c, taps, mode)
        h = taps // 2
        hb = 0 if mode == 0 else 16 * ((h + 15) // 16)
        off = 0 if mode == 0 else hb - h
        assert nb == (1 if 31 + off + taps - 1 < 64 else 2), (taps, nb)
        assert csum == int(c.sum()) and hi == int(((c < -128) | (c > 127)).any()), (taps, csum, hi)
        img = rng.integers(-128, 128, 1024)                                # the wave's image: 1 KB of signed bytes
        got = _toeplitz_from_frags(frags, nb, img)
        want = np.array([int((c * img[u + off:u + off + taps]).sum()) for u in range(512)])
        assert np.array_equal(got, want), (taps, mode)


def test_the_k_block_edge_sits_between_33_and_35_taps_and_single_digit_sets_say_so():
    assert _frags(np.ones(33), 33, 1)[0] == 1 and _frags(np.ones(35), 35, 1)[0] == 2
    assert _frags(np.ones(33), 33, 0)[0] == 1 and _frags(np.ones(35), 35, 0)[0] == 2
    assert _frags(np.full(9, 127), 9, 1)[3] == 0 and _frags(np.full(9, -128), 9, 1)[3] == 0
    assert _frags([0] * 8 + [128], 9, 1)[3] == 1 and _frags([-129] + [0] * 8, 9, 1)[3] == 1
    assert _frags([32640] + [0] * 8, 9, 1)[0] == 0                        # the balanced high digit would be 128
    assert _frags(np.ones(67), 67, 1)[0] == 0


def test_the_int16_geometry_is_unchanged_by_the_parameter():
    # halos rounded to 8: 11 taps start 3 samples into the image (h = 5, hb = 8); rounded to 16 they start 11 samples in
    c = np.arange(1, 12)
    _, f8, _, _ = _frags(c, 11, 1, in_bytes=0)
    _, f16, _, _ = _frags(c, 11, 1, in_bytes=1)
    row0_8 = f8[:4 * 64].view(np.int8).reshape(64, 16)
    row0_16 = f16[:4 * 64].view(np.int8).reshape(64, 16)
    assert list(row0_8[0][:14]) == [0, 0, 0] + list(range(1, 12))         # lane 0: row 0, K 0 .. 15
    assert list(row0_16[0][:16]) == [0] * 11 + [1, 2, 3, 4, 5]
