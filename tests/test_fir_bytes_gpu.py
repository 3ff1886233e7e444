"""GPU parity tests, byte samples (ACDSP_FLAG_IN_BYTES, fir_s8.hip): the HIP engine on 1-byte input containers against the CPU oracle, bit for bit.

Types unless a case says otherwise: IN <8,2> signed, COEFF <16,2>, ACC <48,28> (F = 20 = F_in + F_coeff; 2^36 is the largest possible sum),
OUT <16,I_o,RND,SAT> with I_o = 6 up to 33 taps, 8 up to 255, 9 up to 2049, 10 at 4097 and 11 at 16384.  A stream is n_taps + 2 * 1024 + 77
samples and is compared whole; every case asserts that the oracle's saturated share past the first n_taps outputs is at most 20 %, the three
"must saturate" cases (I_o = 7 at 255 taps, 8 at 2049, 10 at 16384) that it is above 0.

mfma_issued() is nb + (hb1 - hb0 + 1) with nb = max(2, ceil((n_taps - 1) / 32) + 1) K-blocks (long_blocks) and [hb0, hb1] the K-blocks that
hold a non-zero high coefficient byte: 2 nb on a dense set of at least two taps.  ONE tap sits in K-block nb - 1 alone (block 0 holds taps
1 .. 63 of the reach), so a one-tap filter issues nb + 1 = 3."""
import struct

import numpy as np
import pytest
import torch

import ac_dsp_amd as A
from oracle import OracleFir
from helpers import ofmt, windowed_sinc
from test_fir_gpu import rand_raw
from test_graph_gpu import _capture_and_check

pytestmark = pytest.mark.gpu

F8 = A.Fmt(8, 2)
FC = A.Fmt(16, 2)
FA = A.Fmt(48, 28)


def fo_for(n_taps, drop=0):
    i_o = 6 if n_taps <= 33 else (8 if n_taps <= 255 else (9 if n_taps <= 2049 else (10 if n_taps <= 4097 else 11)))
    return A.Fmt(16, i_o - drop, True, "RND", "SAT")


def stream_len(n_taps):
    return n_taps + 2 * 1024 + 77


def dense(n_taps, seed=1):
    return np.random.default_rng(seed).integers(-32768, 32640, size=n_taps, dtype=np.int64)


def n_blocks(n_taps):
    return max(2, (n_taps - 1 + 31) // 32 + 1)


def sat_share(yo, fo, n_taps):
    """share of the oracle's outputs past the first n_taps that sit on a bound of OUT_TYPE"""
    lo = -(1 << (fo.W - 1)) if fo.S else 0
    hi = (1 << (fo.W - 1)) - 1 if fo.S else (1 << fo.W) - 1
    tail = yo[:, n_taps:]
    return float(np.mean((tail == lo) | (tail == hi)))


def check_share(yo, fo, n_taps, what="", want_sat=False):
    """the convention of every case: at most 20 % of the oracle's outputs past the fill sit on a bound of OUT_TYPE"""
    share = sat_share(yo, fo, n_taps)
    print("%s %d taps: saturated share past the fill %.4f" % (what, n_taps, share))
    assert share <= 0.20, (what, share)
    if want_sat:
        assert share > 0, (what, share)


def same(y, yo, what=""):
    assert y.shape == yo.shape, (what, y.shape, yo.shape)
    bad = np.argwhere(y != yo)
    assert bad.size == 0, "%s: %d mismatches, first at %s: got %d want %d" % (what, len(bad), bad[0], y[tuple(bad[0])], yo[tuple(bad[0])])


def run_bytes(fir, x, splits=None):
    """test_fir_gpu.run_engine with the rows converted to the handle's own input containers (Fir.in_dtype)"""
    dt = fir.in_dtype
    outs = []
    bounds = [0] + list(splits or []) + [x.shape[1]]
    for a, b in zip(bounds[:-1], bounds[1:]):
        if b == a:
            continue
        xd = torch.from_numpy(x[:, a:b].copy()).to(dt).cuda()
        outs.append(fir.run(xd).cpu().numpy().astype(np.int64))
    return np.concatenate(outs, axis=1)


def oracle_of(n_taps, ftype, fin, fc, fa, fo, n_ch, reg_share=False):
    kw = dict(reg_share=(1, 1, 0)) if reg_share else {}
    return OracleFir(n_taps, ftype, ofmt(fin), ofmt(fc), ofmt(fa), ofmt(fo), n_ch=n_ch, **kw)


def bytes_case(n_taps, coeffs, ftype="SHIFT_REG", fin=F8, fc=FC, fa=FA, fo=None, n_ch=3, kind="load", splits_list=((),), seed=0, x=None,
               reg_share=False, expect_path="mfma_s8", want_sat=False, per_channel=False, force_generic=False, check_sat=True):
    """one oracle run, one engine stream per call pattern; returns (last engine handle, x, oracle output)"""
    fo = fo or fo_for(n_taps)
    if x is None:
        x = rand_raw(np.random.default_rng(seed), fin, (n_ch, stream_len(n_taps)))
    yo = oracle_of(n_taps, ftype, fin, fc, fa, fo, n_ch, reg_share).run(coeffs, x)
    if check_sat:
        check_share(yo, fo, n_taps, ftype, want_sat)
    fir = None
    for splits in splits_list:
        fir = A.Fir(n_taps, ftype, fin, fc, fa, fo, n_channels=n_ch, kind="reg_share" if reg_share else kind, in_bytes=True,
                    coeffs_per_channel=per_channel, force_generic=force_generic)
        fir.set_coeffs(coeffs)
        if isinstance(expect_path, str):
            assert fir.path == expect_path, fir.path
        else:
            assert fir.path in expect_path, fir.path
        same(run_bytes(fir, x, list(splits)), yo, "%d taps, splits %s" % (n_taps, list(splits)))
    return fir, x, yo


# 1. tap counts and block / segment edges: 33 / 34 taps are the second / third K-block, 481 / 482 the 16th / 17th, 1025 / 1026 the 33rd / 34th:
# the last set whose fragments are resident in LDS and the first that is walked in segments (three of them)
@pytest.mark.parametrize("n_taps", [1, 2, 32, 33, 34, 255, 481, 482, 513, 1025, 1026, 2049, 4097, 16384])
def test_tap_counts_and_block_and_segment_edges(n_taps):
    n_ch = 1 if n_taps == 16384 else 3
    fir, _, _ = bytes_case(n_taps, dense(n_taps), n_ch=n_ch, seed=n_taps,
                           splits_list=(sorted([5, 1040, n_taps + 600]),    # short calls: the history flips buffers
                                        [n_taps + 64]))             # a call of at least hl samples: history written in place
    assert fir.in_dtype == torch.int8
    nb = n_blocks(n_taps)
    assert fir.mfma_issued() == (2 * nb if n_taps >= 2 else nb + 1), (fir.mfma_issued(), nb)   # dense: every K-block that holds a tap has a high byte
    assert fir.mfma_epilogue() is None                              # (-1 off the int8 path)


@pytest.mark.parametrize("n_taps,drop", [(255, 1), (2049, 1), (16384, 1)])
def test_an_output_that_saturates(n_taps, drop):
    n_ch = 1 if n_taps == 16384 else 3
    bytes_case(n_taps, dense(n_taps), fo=fo_for(n_taps, drop), n_ch=n_ch, seed=100 + n_taps, splits_list=([700],), want_sat=True)


# 2. a workgroup is eight channels x at least four pairs of steps: nine channels are two workgroup rows, the second with one live wave and
# seven clamped to its channel; the single call of ten steps is two workgroup columns, the second with one pair, its second step ragged
@pytest.mark.parametrize("n_taps", [255, 1026])
def test_nine_channels_and_two_workgroup_columns(n_taps):
    n_ch = 9
    x = rand_raw(np.random.default_rng(25), F8, (n_ch, 8192 + 1024 + 5))
    bytes_case(n_taps, dense(n_taps), n_ch=n_ch, x=x, splits_list=([], [700, 9000]))


# 3. accumulator bound: every product at its largest magnitude and of one sign, 16384 of them; OUT = ACC
@pytest.mark.parametrize("fin,c,xv", [(F8, -32768, -128), (F8, 32639, 127), (A.Fmt(8, 2, False), -32768, 0), (A.Fmt(8, 2, False), 32639, 255)])
def test_int32_plane_sums_hold_16384_extreme_products(fin, c, xv):
    n_taps = 16384
    x = np.full((1, stream_len(n_taps)), xv, dtype=np.int64)
    fir, _, _ = bytes_case(n_taps, np.full(n_taps, c, dtype=np.int64), fin=fin, fo=FA, n_ch=1, x=x, check_sat=False)
    assert fir.in_dtype == (torch.int8 if fin.S else torch.uint8)
    y_last = run_bytes(fir, x[:, :1])[0, 0]                  # the stream goes on: a full window of extreme products
    assert y_last == n_taps * c * xv, (y_last, n_taps * c * xv)


# 4. high-byte range
def test_high_byte_blocks_outside_the_range_of_the_set_are_not_issued():
    n_taps = 4097
    c = windowed_sinc(n_taps, 0.05, FC)
    fir, _, _ = bytes_case(n_taps, c, fo=A.Fmt(16, 2, True, "RND", "SAT"), splits_list=([n_taps + 64],))
    nb = n_blocks(n_taps)
    assert np.abs(c).max() >= 128 and nb < fir.mfma_issued() < 2 * nb, (fir.mfma_issued(), nb)


def test_a_set_without_a_high_byte_issues_no_high_plane_product():
    n_taps = 8192
    c = windowed_sinc(n_taps, 0.1 * 255 / 8192, FC)
    assert np.abs(c).max() < 128, np.abs(c).max()
    fir, _, _ = bytes_case(n_taps, c, fo=A.Fmt(16, 2, True, "RND", "SAT"), n_ch=2, splits_list=([1000],))
    assert fir.mfma_issued() == n_blocks(n_taps), fir.mfma_issued()


# 5. epilogue at 2049 taps: containers of 2, 4 and 8 bytes, a rounding / overflow pair of the 64-bit epilogue, an accumulator that wraps, an
# unsigned one, unsigned samples (the 128 * sum(c) correction), 4-bit samples in byte containers
# (unsigned samples carry the DC term 127.5 * sum(c): seed 2 is a dense set whose sum, 278127, leaves 6 % of <16,9> saturated; seed 1 leaves 64 %)
@pytest.mark.parametrize("fin,fa,fo,cseed", [
    (F8, FA, A.Fmt(16, 9), 1),
    (F8, FA, A.Fmt(24, 12, True, "RND_CONV", "SAT_SYM"), 1),
    (F8, FA, A.Fmt(48, 28, True, "TRN", "WRAP"), 1),
    (F8, A.Fmt(26, 6), None, 1),                              # F = 20: exact products, the sum wraps the 6 integer bits legitimately
    (F8, A.Fmt(48, 28, False), A.Fmt(48, 28, True, "TRN", "WRAP"), 1),
    (A.Fmt(8, 3, False), FA, None, 2),
    (A.Fmt(4, 1), FA, None, 1),
])
def test_epilogue_types_at_2049_taps(fin, fa, fo, cseed):
    bytes_case(2049, dense(2049, cseed), fin=fin, fa=fa, fo=fo, splits_list=([700],), seed=3, check_sat=fo is None or fo.O != 0)


# the 32-bit epilogue (|V| < 2^30: dense sets of up to ~500 taps) in its variants: AC_TRN, a signed AC_WRAP output, a saturating output of
# fewer than 16 bits, unsigned samples; and an output row that takes no 16-byte store
@pytest.mark.parametrize("fin,fo,cseed", [
    (F8, A.Fmt(16, 8, True, "TRN", "SAT"), 1),
    (F8, A.Fmt(12, 3, True, "RND", "WRAP"), 1),
    (F8, A.Fmt(14, 8, True, "RND", "SAT"), 1),
    (A.Fmt(8, 3, False), A.Fmt(16, 9, True, "RND", "SAT"), 1),
    (A.Fmt(4, 1), A.Fmt(16, 7, True, "RND", "SAT"), 1),
])
def test_epilogue_types_at_255_taps(fin, fo, cseed):
    bytes_case(255, dense(255, cseed), fin=fin, fo=fo, splits_list=([700], [1024]), seed=4, check_sat=fo.O != 0)


# calls of at least 4096 samples: the whole pairs run the branch-free instantiation of the one-segment form, the rest the general one behind
# it.  Nine channels: the second workgroup row has seven waves on the last channel's rows
# (cseed None: a windowed-sinc set, whose sum |c| keeps the 32-bit epilogue -- and with it the branch-free instantiation -- at 1023 taps; the
# dense sets of 513 and 1025 taps, the largest resident one, run the general kernel without a barrier)
@pytest.mark.parametrize("n_taps,fin,cseed", [(2, F8, 1), (34, F8, 1), (255, F8, 1), (481, F8, 1), (255, A.Fmt(8, 3, False), 1),
                                              (513, F8, 1), (1023, F8, None), (1025, F8, 1)])
def test_whole_pairs_of_the_one_segment_form(n_taps, fin, cseed):
    n_ch = 9
    x = rand_raw(np.random.default_rng(70 + n_taps), fin, (n_ch, 3 * 4096 + 2048 + 5))
    fo = A.Fmt(16, 9, True, "RND", "SAT") if not fin.S else fo_for(n_taps)
    c = dense(n_taps, cseed) if cseed is not None else windowed_sinc(n_taps, 0.05, FC)
    if cseed is None:
        fo = A.Fmt(16, 2, True, "RND", "SAT")
    bytes_case(n_taps, c, fin=fin, fo=fo, n_ch=n_ch, x=x, splits_list=([], [100, 100 + 4096]))


def test_output_rows_that_take_no_16_byte_store():
    n_taps, n_ch = 255, 3
    c = dense(n_taps)
    x = rand_raw(np.random.default_rng(41), F8, (n_ch, stream_len(n_taps)))
    fo = fo_for(n_taps)
    yo = oracle_of(n_taps, "SHIFT_REG", F8, FC, FA, fo, n_ch).run(c, x)
    check_share(yo, fo, n_taps, "misaligned output rows")
    fir = A.Fir(n_taps, "SHIFT_REG", F8, FC, FA, fo, n_channels=n_ch, kind="load", in_bytes=True)
    fir.set_coeffs(c)
    out = torch.zeros((n_ch, x.shape[1] + 3), dtype=torch.int16, device="cuda")[:, 1:]      # rows 2 bytes off, stride 2383 = 7 mod 8
    y = fir.run(torch.from_numpy(x).to(torch.int8).cuda(), out=out)
    same(y[:, :x.shape[1]].cpu().numpy().astype(np.int64), yo, "misaligned output rows")


# 6. kinds and FTYPEs
@pytest.mark.parametrize("ftype,n_taps,kind", [("FOLD_EVEN", 256, "load"), ("FOLD_ODD", 255, "prog"), ("C_BUFF", 255, "load"),
                                               ("ROTATE_SHIFT", 255, "prog"), ("TRANSPOSED", 255, "const"), ("FOLD_ODD", 4097, "prog")])
def test_architectures(ftype, n_taps, kind):
    bytes_case(n_taps, dense(n_taps, seed=7), ftype=ftype, kind=kind, splits_list=([333, 1500],), seed=n_taps)


def test_reg_share_at_2049_taps():
    bytes_case(2049, dense(2049, seed=8), ftype="SHIFT_REG", reg_share=True, splits_list=([333, 1500],), seed=9)


# 7. rows: byte rows may start anywhere as long as a row is readable up to the next multiple of 16 bytes; else the staging image
def _run_rows(make_rows, what):
    n_taps, n_ch = 255, 3
    n = stream_len(n_taps)
    c = dense(n_taps, seed=30)
    x = rand_raw(np.random.default_rng(31), F8, (n_ch, n))
    fo = fo_for(n_taps)
    yo = oracle_of(n_taps, "SHIFT_REG", F8, FC, FA, fo, n_ch).run(c, x)
    check_share(yo, fo, n_taps, what)
    fir = A.Fir(n_taps, "SHIFT_REG", F8, FC, FA, fo, n_channels=n_ch, kind="load", in_bytes=True)
    fir.set_coeffs(c)
    assert fir.path == "mfma_s8"
    xd = make_rows(torch.from_numpy(x).to(torch.int8), n_ch, n)
    assert xd.shape == (n_ch, n) and xd.stride(1) == 1
    same(fir.run(xd).cpu().numpy().astype(np.int64), yo, what)


def test_a_row_stride_that_is_no_multiple_of_16():
    def rows(x, n_ch, n):
        buf = torch.zeros((n_ch, (n + 15) // 16 * 16 + 5), dtype=torch.int8, device="cuda")
        buf[:, :n] = x.cuda()
        return buf[:, :n]
    _run_rows(rows, "row stride 2389")


def test_a_view_that_starts_one_byte_into_its_allocation():
    def rows(x, n_ch, n):
        stride = (n + 15) // 16 * 16 + 16
        flat = torch.zeros(n_ch * stride + 16, dtype=torch.int8, device="cuda")
        v = flat[1:1 + n_ch * stride].view(n_ch, stride)[:, :n]
        v.copy_(x.cuda())
        assert v.data_ptr() % 16 == 1
        return v
    _run_rows(rows, "rows one byte off")


def test_a_last_row_that_ends_with_its_allocation_goes_through_the_staging_image():
    def rows(x, n_ch, n):
        assert n % 16 != 0
        return x.cuda().contiguous()                          # stride n: the last row is not readable up to the next multiple of 16
    _run_rows(rows, "dense rows")


# 8. flagged handles off the new path: the exact-order kernels read the byte rows through load_raw
def test_a_coefficient_set_per_channel_runs_the_exact_order_kernels():
    c = rand_raw(np.random.default_rng(50), FC, (3, 63))
    bytes_case(63, c, fo=fo_for(63), per_channel=True, expect_path=("generic", "lossless64"), splits_list=([5, 300],), seed=51)


def test_a_lossy_accumulator_runs_the_exact_order_kernel():
    bytes_case(127, dense(127), fa=A.Fmt(40, 30), expect_path=("generic",), splits_list=([5, 300],), seed=52)


def test_force_generic_equals_the_unforced_handle():
    c = dense(255, seed=53)
    _, x, yo = bytes_case(255, c, splits_list=([100],), seed=54)
    bytes_case(255, c, x=x, force_generic=True, expect_path=("generic", "lossless64"), splits_list=([100],))


def test_a_coefficient_that_does_not_split_into_two_signed_bytes():
    c = dense(2049)
    c[100] = 32700
    bytes_case(255, c[:255], expect_path=("lossless64",), splits_list=([100],), seed=55)
    fir = A.Fir(2049, "SHIFT_REG", F8, FC, FA, fo_for(2049), n_channels=1, kind="load", in_bytes=True)
    with pytest.raises(A.AcdspError) as e:
        fir.set_coeffs(c)
    assert e.value.code == 2, e.value                         # ACDSP_EUNSUPPORTED
    with pytest.raises(A.AcdspError) as e:                    # the handle is left without a set
        fir.run(torch.zeros((1, 64), dtype=torch.int8, device="cuda"))
    assert e.value.code == 5, e.value                         # ACDSP_ESTATE


# 9. state
def test_state_blobs_clone_reset_and_run_host():
    n_taps, n_ch = 255, 3
    fo = fo_for(n_taps)
    c = dense(n_taps, seed=60)
    rng = np.random.default_rng(61)
    x = [rand_raw(rng, F8, (n_ch, n)) for n in (700, 300, 1100, 500)]

    def mk(**kw):
        kw.setdefault("in_bytes", True)
        f = A.Fir(n_taps, "SHIFT_REG", F8, FC, FA, fo, n_channels=n_ch, kind="load", **kw)
        f.set_coeffs(c)
        return f

    orc = oracle_of(n_taps, "SHIFT_REG", F8, FC, FA, fo, n_ch)
    fast, slow = mk(), mk(force_generic=True)
    assert fast.path == "mfma_s8" and slow.path != "mfma_s8"
    want = orc.run(c, x[0])
    check_share(want, fo, n_taps, "state, first call")
    same(run_bytes(fast, x[0]), want, "first call")
    same(run_bytes(slow, x[0]), want, "first call, force_generic")
    blob = fast.state()
    assert struct.unpack_from("<I", blob, 20)[0] == 1, "elem_bytes of the state header"
    assert len(blob) == 64 + n_ch * 288                       # hl = 288 one-byte words per channel
    # mid-stream into a handle of the other path, both ways
    into_slow, into_fast = mk(force_generic=True), mk()
    into_slow.set_state(blob)
    into_fast.set_state(slow.state())
    # a blob of an unflagged twin (int16 containers) is refused and leaves the handle as it was
    twin16 = mk(in_bytes=False)
    twin16.run(torch.from_numpy(x[0]).to(torch.int16).cuda())
    with pytest.raises(A.AcdspError) as e:
        fast.set_state(twin16.state())
    assert e.value.code == 1, e.value                         # ACDSP_EINVAL
    cl = fast.clone()
    want = orc.run(c, x[1])
    check_share(want, fo, 0, "state, second call")
    for f, what in ((fast, "stream, after the refused blob"), (into_slow, "mfma_s8 blob in a force_generic handle"),
                    (into_fast, "force_generic blob in an mfma_s8 handle"), (cl, "clone")):
        same(run_bytes(f, x[1], [17]), want, what)
    assert cl.path == "mfma_s8" and cl.in_dtype == torch.int8
    want = orc.run(c, x[2])
    check_share(want, fo, 0, "state, third call")
    same(run_bytes(fast, x[2]), want, "stream, third call")
    want_cl = oracle_of(n_taps, "SHIFT_REG", F8, FC, FA, fo, n_ch)
    want_cl.run(c, np.concatenate([x[0], x[1]], axis=1))
    same(run_bytes(cl, x[3]), want_cl.run(c, x[3]), "clone on its own")
    fast.reset()
    fresh = oracle_of(n_taps, "SHIFT_REG", F8, FC, FA, fo, n_ch)
    same(run_bytes(fast, x[3]), fresh.run(c, x[3]), "after reset()")
    host = mk()
    same(host.run_host(x[3]).astype(np.int64), oracle_of(n_taps, "SHIFT_REG", F8, FC, FA, fo, n_ch).run(c, x[3]), "run_host")
    big = rand_raw(rng, F8, (n_ch, 40000))                    # past the pinned buffers: the staged device image
    a, b = mk(), mk()
    same(a.run_host(big).astype(np.int64), run_bytes(b, big), "run_host against run")


# 10. graph capture
@pytest.mark.parametrize("n_taps", [255, 2049])
def test_byte_fir_calls_replayed_from_a_graph_continue_the_stream(n_taps):
    nch, cs, nk = 8, 4096, 3
    c = dense(n_taps, seed=23)
    fo = fo_for(n_taps)

    def make():
        e = A.Fir(n_taps, "SHIFT_REG", F8, FC, FA, fo, n_channels=nch, kind="load", in_bytes=True)
        e.set_coeffs(c)
        assert e.path == "mfma_s8"
        return e

    rng = np.random.default_rng(24)
    x = torch.from_numpy(rng.integers(-128, 128, size=(nk, nch, cs), dtype=np.int8)).cuda()
    y0 = make().run(x[0]).cpu().numpy().astype(np.int64)      # one eager call of the same shape first, against the oracle
    want = oracle_of(n_taps, "SHIFT_REG", F8, FC, FA, fo, nch).run(c, x[0].cpu().numpy().astype(np.int64))
    check_share(want, fo, n_taps, "graph, eager call")
    same(y0, want, "eager call")
    _capture_and_check(make, x, (nch, cs), torch.int16)


# 11. node layer
def test_node_layer_shards_byte_rows():
    n_taps, n_ch = 255, 7
    c = dense(n_taps, seed=21)
    fo = fo_for(n_taps)
    rng = np.random.default_rng(22)
    node = A.NodeFir(n_taps, "SHIFT_REG", F8, FC, FA, fo, n_ch, [0, 0, 0], kind="load", in_bytes=True)
    node.set_coeffs(c)
    assert node.slices == [(0, 3), (3, 5), (5, 7)]
    orc = oracle_of(n_taps, "SHIFT_REG", F8, FC, FA, fo, n_ch)
    for n in (1300, 1024):
        x = rand_raw(rng, F8, (n_ch, n))
        xs = [torch.from_numpy(x[lo:hi].copy()).to(torch.int8).cuda() for lo, hi in node.slices]
        ys = node.run(xs)
        torch.cuda.synchronize()
        want = orc.run(c, x)
        check_share(want, fo, n_taps if n == 1300 else 0, "node call of %d samples" % n)
        same(np.concatenate([y.cpu().numpy().astype(np.int64) for y in ys]), want, "node call of %d samples" % n)
    x = rand_raw(rng, F8, (n_ch, 777))
    same(node.run_host(x).astype(np.int64), orc.run(c, x), "node run_host")
    node.close()
