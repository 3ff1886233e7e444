"""GPU parity tests, long FIRs (1026 .. 16384 taps, fir_long.hip): the HIP engine against the CPU oracle, bit for bit.

Every 16384-tap tap must see data, so a case streams n = n_taps + 2 * 1024 + 77 samples and compares the whole stream.  Dense full-range
sets into OUT <16,10,RND,SAT> saturate at most 0.1 % of the outputs past the fill (into <16,2> they would saturate 95 % and hide everything);
every case asserts that the oracle's saturated share past the first n_taps outputs is at most 20 %."""
import ctypes as C

import numpy as np
import pytest
import torch

import ac_dsp_amd as A
from ac_dsp_amd._lib import lib, check
from oracle import OracleFir
from helpers import ofmt, windowed_sinc
from test_fir_gpu import rand_raw, run_engine
from test_graph_gpu import _capture_and_check

pytestmark = pytest.mark.gpu

F16 = A.Fmt(16, 2)
FA = A.Fmt(48, 20)                          # F = 28 = F_in + F_coeff: exact products, 19 integer bits of headroom
FO = A.Fmt(16, 10, True, "RND", "SAT")
SB = 16                                     # K-blocks per LDS segment of the kernel (fir_long_kernels.hpp: kLongSB)


def stream_len(n_taps):
    return n_taps + 2 * 1024 + 77


def dense(n_taps, seed=1):
    return np.random.default_rng(seed).integers(-32768, 32640, size=n_taps, dtype=np.int64)


def n_blocks(n_taps):
    return (n_taps - 1 + 31) // 32 + 1


def sat_share(yo, fo, n_taps):
    """share of the oracle's outputs past the first n_taps that sit on a bound of OUT_TYPE"""
    lo = -(1 << (fo.W - 1)) if fo.S else 0
    hi = (1 << (fo.W - 1)) - 1 if fo.S else (1 << fo.W) - 1
    tail = yo[:, n_taps:]
    return float(np.mean((tail <= lo + 1) | (tail >= hi)))


def same(y, yo, what=""):
    bad = np.argwhere(y != yo)
    assert bad.size == 0, "%s: %d mismatches, first at %s: got %d want %d" % (what, len(bad), bad[0], y[tuple(bad[0])], yo[tuple(bad[0])])


def long_case(n_taps, ftype, fin, fc, fa, fo, coeffs, n_ch=3, kind="load", splits_list=((),), seed=0, x=None, reg_share=False,
              expect_path="mfma_long", want_sat=False):
    """one oracle run, one engine stream per call pattern; returns the last engine handle"""
    rng = np.random.default_rng(seed)
    if x is None:
        x = rand_raw(rng, fin, (n_ch, stream_len(n_taps)))
    kw = dict(reg_share=(1, 1, 0)) if reg_share else {}
    yo = OracleFir(n_taps, ftype, ofmt(fin), ofmt(fc), ofmt(fa), ofmt(fo), n_ch=n_ch, **kw).run(coeffs, x)
    share = sat_share(yo, fo, n_taps)
    print("%d taps %s: saturated share past the fill %.4f" % (n_taps, ftype, share))
    assert share <= 0.20, share
    if want_sat:
        assert share > 0, share
    fir = None
    for splits in splits_list:
        fir = A.Fir(n_taps, ftype, fin, fc, fa, fo, n_channels=n_ch, kind="reg_share" if reg_share else kind)
        fir.set_coeffs(coeffs)
        assert fir.path == expect_path, fir.path
        same(run_engine(fir, x, list(splits)), yo, "%d taps, splits %s" % (n_taps, list(splits)))
    return fir


# 1. tap counts and segment edges.  A new segment begins with K-block 16 k: NB = 16 k + 1 from 512 k - 30 taps on (1505 / 1506 with k = 3);
# 512 k + 1 +- 1 (1536 / 1538) put the last tap one into, and one short of, the next K-block of the reach 32 * 16 k.
@pytest.mark.parametrize("n_taps", [1026, 1057, 1058, 32 * SB * 3 - 31, 32 * SB * 3 - 30, 32 * SB * 3, 32 * SB * 3 + 2, 2048, 2049, 4097, 8192, 16384])
def test_tap_counts_and_segment_edges(n_taps):
    n_ch = 1 if n_taps == 16384 else (2 if n_taps == 8192 else 3)
    fir = long_case(n_taps, "SHIFT_REG", F16, F16, FA, FO, dense(n_taps), n_ch=n_ch, seed=n_taps,
                    splits_list=([5, 1040, n_taps + 600],    # short calls: the history flips buffers
                                 [n_taps + 64]))             # a call of at least hl samples: history written in place
    assert fir.mfma_issued() == 4 * n_blocks(n_taps)         # dense: every high-byte block is issued
    assert fir.mfma_epilogue() is None                       # (-1 off the int8 path)


# a workgroup is eight channels x at least eight steps: nine channels are two workgroup rows, the second with one live wave and seven
# clamped to its channel; the single call of ten steps is two workgroup columns, the second with two steps, the last of them ragged
def test_nine_channels_and_two_workgroup_columns():
    n_ch = 9
    x = rand_raw(np.random.default_rng(25), F16, (n_ch, 8192 + 1024 + 5))
    long_case(1026, "SHIFT_REG", F16, F16, FA, FO, dense(1026), n_ch=n_ch, x=x, splits_list=([], [700, 9000]))


# 2. accumulator bound: every product at its largest magnitude and of one sign, 16384 of them
@pytest.mark.parametrize("c,xv", [(-32768, -32768), (32639, 32767)])
def test_int32_plane_sums_hold_16384_extreme_products(c, xv):
    n_taps = 16384
    x = np.full((1, stream_len(n_taps)), xv, dtype=np.int64)
    fir = long_case(n_taps, "SHIFT_REG", F16, F16, FA, FA, np.full(n_taps, c, dtype=np.int64), n_ch=1, x=x)
    y_last = run_engine(fir, x[:, :1])[0, 0]                 # the stream goes on: a full window of extreme products
    assert y_last == n_taps * c * xv, (y_last, n_taps * c * xv)


# 3. high-byte range
def test_high_byte_blocks_outside_the_range_of_the_set_are_not_issued():
    n_taps = 4097
    c = windowed_sinc(n_taps, 0.05, F16)
    fir = long_case(n_taps, "SHIFT_REG", F16, F16, FA, A.Fmt(16, 2, True, "RND", "SAT"), c, splits_list=([n_taps + 64],))
    nb = n_blocks(n_taps)
    assert np.abs(c).max() >= 128 and 2 * nb < fir.mfma_issued() < 4 * nb, (fir.mfma_issued(), nb)


def test_a_set_without_a_high_byte_issues_no_high_plane_product():
    n_taps = 8192
    c = windowed_sinc(n_taps, 0.1 * 255 / 8192, F16)
    assert np.abs(c).max() < 128, np.abs(c).max()
    fir = long_case(n_taps, "SHIFT_REG", F16, F16, FA, A.Fmt(16, 2, True, "RND", "SAT"), c, n_ch=2, splits_list=([1000],))
    assert fir.mfma_issued() == 2 * n_blocks(n_taps), fir.mfma_issued()


# 4. epilogue: containers of 2, 4 and 8 bytes, an accumulator that wraps, an unsigned one, an output that saturates
@pytest.mark.parametrize("fa,fo", [
    (FA, A.Fmt(16, 10)),
    (FA, A.Fmt(24, 12, True, "RND_CONV", "SAT_SYM")),
    (FA, A.Fmt(48, 20, True, "TRN", "WRAP")),
    (A.Fmt(34, 6), FO),                                       # F = 28: exact products, the sum wraps the 6 integer bits legitimately
    (A.Fmt(48, 20, False), A.Fmt(48, 20, True, "TRN", "WRAP")),
])
def test_epilogue_types_at_2049_taps(fa, fo):
    long_case(2049, "SHIFT_REG", F16, F16, fa, fo, dense(2049), splits_list=([700],), seed=3)


def test_an_output_that_saturates_at_8192_taps():
    long_case(8192, "SHIFT_REG", F16, F16, FA, A.Fmt(16, 9, True, "RND", "SAT"), dense(8192), n_ch=2, splits_list=([3000],), seed=4, want_sat=True)


# 5. types and architectures
@pytest.mark.parametrize("ftype,n_taps,kind", [("FOLD_EVEN", 4096, "load"), ("FOLD_ODD", 4097, "prog"), ("C_BUFF", 2049, "load"),
                                               ("ROTATE_SHIFT", 2049, "prog"), ("TRANSPOSED", 2049, "const")])
def test_architectures(ftype, n_taps, kind):
    n_ch = 1 if ftype == "ROTATE_SHIFT" else 3               # (the oracle rotates its register per sample: ~20 x the time of the other ftypes)
    long_case(n_taps, ftype, F16, F16, FA, FO, dense(n_taps, seed=7), n_ch=n_ch, kind=kind, splits_list=([333, 1500],), seed=n_taps)


def test_reg_share_anti_symmetric_fold():
    c = np.clip(dense(2050, seed=8), -32000, 32000)          # the negated mirror half must stay below 32640 too
    long_case(2050, "FOLD_EVEN_ANTI", F16, F16, FA, FO, c, reg_share=True, splits_list=([333, 1500],), seed=9)


def test_unsigned_16_bit_samples():
    # the DC term 32768 * sum(c) of a dense set would saturate <16,10>: a 24-bit output keeps every word visible
    long_case(2049, "SHIFT_REG", A.Fmt(16, 3, False), F16, FA, A.Fmt(24, 12, True, "RND", "SAT"), dense(2049, seed=10), splits_list=([1, 2500],), seed=11)


def test_narrow_samples_and_coefficients_at_3000_taps():
    fin, fc = A.Fmt(12, 4), A.Fmt(10, 2)
    c = rand_raw(np.random.default_rng(12), fc, (3000,))
    long_case(3000, "SHIFT_REG", fin, fc, FA, A.Fmt(24, 12, True, "RND", "SAT"), c, splits_list=([77],), seed=13)


# 6. saturating accumulators
def test_a_saturating_accumulator_that_cannot_saturate_runs_the_long_kernel():
    long_case(4097, "SHIFT_REG", F16, F16, A.Fmt(40, 12, True, "TRN", "SAT"), FO, windowed_sinc(4097, 0.05, F16), splits_list=([4097 + 64],), seed=14)


def test_a_saturating_accumulator_that_may_saturate_is_refused_above_2048_taps_and_runs_as_before_below():
    fa = A.Fmt(40, 12, True, "TRN", "SAT")
    n_taps = 4097
    fir = A.Fir(n_taps, "SHIFT_REG", F16, F16, fa, FO, n_channels=2, kind="load")
    with pytest.raises(A.AcdspError) as e:
        fir.set_coeffs(dense(n_taps))
    assert e.value.code == 2, e.value
    x = rand_raw(np.random.default_rng(15), F16, (2, 1500))
    with pytest.raises(A.AcdspError):                        # the handle is left without a set
        run_engine(fir, x)
    c = windowed_sinc(n_taps, 0.05, F16)
    fir.set_coeffs(c)
    assert fir.path == "mfma_long"
    same(run_engine(fir, x, [200]), OracleFir(n_taps, "SHIFT_REG", ofmt(F16), ofmt(F16), ofmt(fa), ofmt(FO), n_ch=2).run(c, x), "after the refusal")
    # 2047 taps: the same dense set keeps today's exact-order path
    fir = A.Fir(2047, "SHIFT_REG", F16, F16, fa, FO, n_channels=2, kind="load")
    fir.set_coeffs(dense(2047))
    assert fir.path != "mfma_long"
    x = rand_raw(np.random.default_rng(16), F16, (2, 2047 + 300))
    same(run_engine(fir, x, [100]), OracleFir(2047, "SHIFT_REG", ofmt(F16), ofmt(F16), ofmt(fa), ofmt(FO), n_ch=2).run(dense(2047), x), "2047 taps")


def test_a_coefficient_that_does_not_split_into_two_signed_bytes():
    c = dense(2049)
    c[100] = 32700
    fir = A.Fir(2049, "SHIFT_REG", F16, F16, FA, FO, n_channels=1, kind="load")
    with pytest.raises(A.AcdspError) as e:
        fir.set_coeffs(c)
    assert e.value.code == 2, e.value
    # up to 2048 taps such a set keeps the exact-sum VALU kernel
    fir = A.Fir(1100, "SHIFT_REG", F16, F16, FA, FO, n_channels=1, kind="load")
    fir.set_coeffs(c[:1100])
    assert fir.path == "lossless64", fir.path
    x = rand_raw(np.random.default_rng(17), F16, (1, 1500))
    same(run_engine(fir, x), OracleFir(1100, "SHIFT_REG", ofmt(F16), ofmt(F16), ofmt(FA), ofmt(FO), n_ch=1).run(c[:1100], x), "1100 taps")


# 7. stream state at 4097 taps, kind load
def _clone(fir):
    other = A.Fir.__new__(A.Fir)
    other.__dict__.update({k: v for k, v in fir.__dict__.items() if k != "_h"})
    other._h = C.c_void_p()
    check(lib.acdsp_fir_clone(fir._h, C.byref(other._h)))
    return other


def test_stream_state_at_4097_taps():
    n_taps, n_ch = 4097, 3
    rng = np.random.default_rng(18)
    mk = lambda: A.Fir(n_taps, "SHIFT_REG", F16, F16, FA, FO, n_channels=n_ch, kind="load")
    orc = OracleFir(n_taps, "SHIFT_REG", ofmt(F16), ofmt(F16), ofmt(FA), ofmt(FO), n_ch=n_ch)
    fir = mk()
    c1, c2 = dense(n_taps, seed=19), dense(n_taps, seed=20)
    x = [rand_raw(rng, F16, (n_ch, n)) for n in (1500, 900, 4200, 1100, 2000)]
    fir.set_coeffs(c1)
    same(run_engine(fir, x[0]), orc.run(c1, x[0]), "first call")
    fir.set_coeffs(c2)                                        # a coefficient change between calls
    same(run_engine(fir, x[1]), orc.run(c2, x[1]), "after a coefficient change")
    other = mk()                                              # state() / set_state() into a second handle, mid-stream
    other.set_coeffs(c2)
    other.set_state(fir.state())
    twin = _clone(fir)                                        # and a deep copy of the handle
    want = orc.run(c2, x[2])
    for f, what in ((fir, "stream"), (other, "after a state load"), (twin, "clone")):
        same(run_engine(f, x[2], [17]), want, what)
        assert f.path == "mfma_long"
    want = orc.run(c2, x[3])
    same(run_engine(fir, x[3]), want, "stream, fourth call")
    same(run_engine(twin, x[3]), want, "clone, fourth call")
    fir.reset()
    same(run_engine(fir, x[4]), OracleFir(n_taps, "SHIFT_REG", ofmt(F16), ofmt(F16), ofmt(FA), ofmt(FO), n_ch=n_ch).run(c2, x[4]), "after reset()")


def test_node_layer_shards_a_long_filter():
    n_taps, n_ch = 4097, 6
    c = dense(n_taps, seed=21)
    rng = np.random.default_rng(22)
    node = A.NodeFir(n_taps, "SHIFT_REG", F16, F16, FA, FO, n_ch, [0, 0], kind="load")
    node.set_coeffs(c)
    assert node.slices == [(0, 3), (3, 6)]
    orc = OracleFir(n_taps, "SHIFT_REG", ofmt(F16), ofmt(F16), ofmt(FA), ofmt(FO), n_ch=n_ch)
    for n in (1300, 1024):
        x = rand_raw(rng, F16, (n_ch, n))
        xs = [torch.from_numpy(x[lo:hi].copy()).to(torch.int16).cuda() for lo, hi in node.slices]
        ys = node.run(xs)
        torch.cuda.synchronize()
        same(np.concatenate([y.cpu().numpy().astype(np.int64) for y in ys]), orc.run(c, x), "node call of %d samples" % n)
    node.close()


# 8. graph capture
def test_long_fir_calls_replayed_from_a_graph_continue_the_stream():
    n_taps, nch, cs, nk = 2049, 8, 4096, 3
    c = dense(n_taps, seed=23)

    def make():
        e = A.Fir(n_taps, "SHIFT_REG", F16, F16, FA, FO, n_channels=nch, kind="load")
        e.set_coeffs(c)
        assert e.path == "mfma_long"
        return e

    rng = np.random.default_rng(24)
    x = torch.from_numpy(rng.integers(-32768, 32768, size=(nk, nch, cs), dtype=np.int16)).cuda()
    eager = make()
    y0 = eager.run(x[0]).cpu().numpy().astype(np.int64)       # one eager call of the same shape first, against the oracle
    same(y0, OracleFir(n_taps, "SHIFT_REG", ofmt(F16), ofmt(F16), ofmt(FA), ofmt(FO), n_ch=nch).run(c, x[0].cpu().numpy().astype(np.int64)), "eager call")
    _capture_and_check(make, x, (nch, cs), torch.int16)
