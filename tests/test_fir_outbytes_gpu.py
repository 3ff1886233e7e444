"""GPU parity tests, byte outputs (ACDSP_FLAG_OUT_BYTES beside ACDSP_FLAG_IN_BYTES, fir_s8.hip): the HIP engine writing 1-byte output containers
against the CPU oracle, bit for bit.

Types unless a case says otherwise: IN <8,2> signed, COEFF <16,2>, ACC <48,28>, OUT <8,I_o,RND,SAT> with the I_o of test_fir_bytes_gpu.fo_for
(6 up to 33 taps, 8 up to 255, 9 up to 2049, 10 at 4097 and 11 at 16384).  A stream is n_taps + 2 * 1024 + 77 samples and is compared whole;
every AC_SAT case asserts that the oracle's saturated share past the first n_taps outputs is at most 20 %, the "must saturate" cases that it
is above 0.  Every case asserts the output tensor's dtype (Fir.out_dtype) and, unless it names another path, fir.path == "mfma_s8".

Which epilogue a case runs: dense sets of up to ~500 taps and the windowed-sinc set of 1023 taps keep sum|c| max|x| below 2^30 -- the 32-bit
epilogue, 1-byte form (whole pairs of calls of at least 4096 samples on its branch-free instantiation); dense sets from 1025 taps on, the
other rounding / overflow modes and an accumulator that wraps -- the 64-bit epilogue, stored element by element."""
import numpy as np
import pytest
import torch

import ac_dsp_amd as A
from helpers import windowed_sinc
from test_fir_gpu import rand_raw
from test_graph_gpu import _capture_and_check
from test_fir_bytes_gpu import F8, FC, FA, fo_for, stream_len, dense, check_share, same, oracle_of, run_bytes

pytestmark = pytest.mark.gpu


def fo8_for(n_taps, drop=0):
    f = fo_for(n_taps, drop)
    return A.Fmt(8, f.I, True, "RND", "SAT")


def make(n_taps, coeffs, fin=F8, fa=FA, fo=None, n_ch=3, out_bytes=True, **kw):
    fir = A.Fir(n_taps, "SHIFT_REG", fin, FC, fa, fo or fo8_for(n_taps), n_channels=n_ch, kind="load", in_bytes=True, out_bytes=out_bytes, **kw)
    fir.set_coeffs(coeffs)
    return fir


def run_out_bytes(fir, x, splits=None):
    """test_fir_bytes_gpu.run_bytes with the dtype of every output tensor checked against the handle's own output containers"""
    outs = []
    bounds = [0] + list(splits or []) + [x.shape[1]]
    for a, b in zip(bounds[:-1], bounds[1:]):
        if b == a:
            continue
        y = fir.run(torch.from_numpy(x[:, a:b].copy()).to(fir.in_dtype).cuda())
        assert y.dtype == fir.out_dtype and y.dtype == (torch.int8 if fir.fout.S else torch.uint8), (y.dtype, fir.out_dtype)
        outs.append(y.cpu().numpy().astype(np.int64))
    return np.concatenate(outs, axis=1)


def out_bytes_case(n_taps, coeffs, fin=F8, fa=FA, fo=None, n_ch=3, splits_list=((),), seed=0, x=None, expect_path="mfma_s8", want_sat=False,
                   per_channel=False, force_generic=False, check_sat=True):
    """the out_bytes twin of test_fir_bytes_gpu.bytes_case: one oracle run, one engine stream per call pattern under both flags; the handle
    resolves as its twin without the output flag does.  Returns (last engine handle, x, oracle output)"""
    fo = fo or fo8_for(n_taps)
    if x is None:
        x = rand_raw(np.random.default_rng(seed), fin, (n_ch, stream_len(n_taps)))
    yo = oracle_of(n_taps, "SHIFT_REG", fin, FC, fa, fo, n_ch).run(coeffs, x)
    if check_sat:
        check_share(yo, fo, n_taps, "out_bytes", want_sat)
    kw = dict(coeffs_per_channel=per_channel, force_generic=force_generic)
    twin = make(n_taps, coeffs, fin, fa, fo, n_ch, out_bytes=False, **kw)
    assert twin.out_dtype == torch.int16
    fir = None
    for splits in splits_list:
        fir = make(n_taps, coeffs, fin, fa, fo, n_ch, **kw)
        assert fir.path == twin.path and fir.mfma_issued() == twin.mfma_issued(), (fir.path, twin.path, fir.mfma_issued(), twin.mfma_issued())
        if expect_path is not None:
            assert fir.path == expect_path, fir.path
        same(run_out_bytes(fir, x, list(splits)), yo, "%d taps, splits %s" % (n_taps, list(splits)))
    return fir, x, yo


# 1. tap counts: 33 / 34 taps are the second / third K-block, 1025 / 1026 the last resident set and the first that is walked in segments
@pytest.mark.parametrize("n_taps", [1, 2, 33, 34, 255, 1025, 1026, 4097, 16384])
def test_tap_counts(n_taps):
    n_ch = 1 if n_taps == 16384 else 3
    fir, _, _ = out_bytes_case(n_taps, dense(n_taps), n_ch=n_ch, seed=n_taps, splits_list=(sorted([5, 1040, n_taps + 600]), [n_taps + 64]))
    assert fir.in_dtype == torch.int8 and fir.out_dtype == torch.int8


# 2. outputs that saturate
@pytest.mark.parametrize("n_taps,i_o", [(63, 5), (255, 6), (2049, 8), (16384, 10)])
def test_an_output_that_saturates(n_taps, i_o):
    n_ch = 1 if n_taps == 16384 else 3
    out_bytes_case(n_taps, dense(n_taps), fo=A.Fmt(8, i_o, True, "RND", "SAT"), n_ch=n_ch, seed=100 + n_taps, splits_list=([700],), want_sat=True)


# 3. the 32-bit epilogue in its variants: AC_TRN, a signed AC_WRAP output, saturating outputs of fewer than 8 bits, an unsigned output
# (unsigned samples and the set dense(255, 4), whose sum of 238820 lifts the mean into the type), 4-bit samples in byte containers
@pytest.mark.parametrize("fin,fo,cseed,want_sat", [
    (F8, A.Fmt(8, 8, True, "TRN", "SAT"), 1, False),
    (F8, A.Fmt(8, 6, True, "RND", "WRAP"), 1, False),
    (F8, A.Fmt(6, 7, True, "RND", "SAT"), 1, False),
    (F8, A.Fmt(4, 7, True, "RND", "SAT"), 1, False),
    (A.Fmt(8, 3, False), A.Fmt(8, 8, False, "RND", "SAT"), 4, True),
    (A.Fmt(4, 1), A.Fmt(8, 7, True, "RND", "SAT"), 1, False),
])
def test_epilogue_types_at_255_taps(fin, fo, cseed, want_sat):
    out_bytes_case(255, dense(255, cseed), fin=fin, fo=fo, splits_list=([700], [1024]), seed=4, check_sat=fo.O != 0, want_sat=want_sat)


# 4. calls of at least 4096 samples: the whole pairs run the branch-free instantiation, the rest the general one behind it.  Nine channels:
# the second workgroup row has seven waves clamped to the last channel's rows, which repeat that channel's stores
@pytest.mark.parametrize("n_taps,fin,cseed", [(2, F8, 1), (34, F8, 1), (255, F8, 1), (481, F8, 1), (1023, F8, None), (255, A.Fmt(8, 3, False), 1)])
def test_whole_pairs_on_the_branch_free_instantiation(n_taps, fin, cseed):
    n_ch = 9
    x = rand_raw(np.random.default_rng(70 + n_taps), fin, (n_ch, 2 * 4096 + 1024 + 5))
    fo = A.Fmt(8, 9, True, "RND", "SAT") if not fin.S else fo8_for(n_taps)
    c = dense(n_taps, cseed) if cseed is not None else windowed_sinc(n_taps, 0.05, FC)
    if cseed is None:
        fo = A.Fmt(8, 2, True, "RND", "SAT")
    out_bytes_case(n_taps, c, fin=fin, fo=fo, n_ch=n_ch, x=x, splits_list=([], [4096], [700, 9000]))


# 5. output rows and the bytes around them.  "vector": rows on 16-byte boundaries with 16 spare bytes each (16-byte stores: the exchange form
# at 2380 samples, the branch-free instantiation and the exchange form behind it at 5125); the other two take no 16-byte store
@pytest.mark.parametrize("layout,n", [("vector", None), ("vector", 4096 + 1024 + 5), ("one byte off", None), ("stride n + 3", None)])
def test_output_rows_and_the_bytes_between_them(layout, n):
    n_taps, n_ch, sentinel = 255, 3, 0x5A
    n = n or stream_len(n_taps)
    c = dense(n_taps)
    x = rand_raw(np.random.default_rng(41), F8, (n_ch, n))
    fo = fo8_for(n_taps)
    yo = oracle_of(n_taps, "SHIFT_REG", F8, FC, FA, fo, n_ch).run(c, x)
    check_share(yo, fo, n_taps, layout)
    fir = make(n_taps, c)
    assert fir.path == "mfma_s8"
    stride = n + 3 if layout == "stride n + 3" else (n + 15) // 16 * 16 + 16
    off = 1 if layout == "one byte off" else 0
    flat = torch.full((n_ch * stride + 32,), sentinel, dtype=torch.int8, device="cuda")
    assert flat.data_ptr() % 16 == 0
    out = flat[off:off + n_ch * stride].view(n_ch, stride)
    assert out.data_ptr() % 16 == off and (out.stride(0) % 16 == 0) == (layout != "stride n + 3")
    y = fir.run(torch.from_numpy(x).to(torch.int8).cuda(), out=out)
    assert y.dtype == fir.out_dtype
    same(out[:, :n].cpu().numpy().astype(np.int64), yo, layout)
    keep = torch.ones_like(flat, dtype=torch.bool)
    for ch in range(n_ch):
        keep[off + ch * stride:off + ch * stride + n] = False
    assert bool((flat[keep] == sentinel).all()), "%s: a byte outside the output rows was written" % layout
    assert int(keep.sum()) == flat.numel() - n_ch * n


# 6. the 64-bit epilogue with 1-byte stores at 2049 taps: a rounding / overflow pair of its own, an unsigned wrapping output, an accumulator
# that wraps (F = 20: exact products, the sum wraps the 6 integer bits legitimately)
@pytest.mark.parametrize("fa,fo", [
    (FA, A.Fmt(8, 9, True, "RND", "SAT")),
    (FA, A.Fmt(8, 9, True, "RND_CONV", "SAT_SYM")),
    (FA, A.Fmt(8, 8, False, "TRN", "WRAP")),
    (A.Fmt(26, 6), A.Fmt(8, 9, True, "RND", "SAT")),
])
def test_the_64_bit_epilogue_at_2049_taps(fa, fo):
    out_bytes_case(2049, dense(2049), fa=fa, fo=fo, splits_list=([700],), seed=3, check_sat=fo.O != 0)


# 7. both flags off the byte kernel: the exact-order kernels store 1-byte containers through store_raw
def test_a_coefficient_set_per_channel_runs_the_exact_order_kernels():
    c = rand_raw(np.random.default_rng(50), FC, (3, 63))
    fir, _, _ = out_bytes_case(63, c, fo=fo8_for(63), per_channel=True, expect_path=None, splits_list=([5, 300],), seed=51)
    assert fir.path in ("generic", "lossless64"), fir.path


def test_force_generic_runs_the_exact_order_kernels():
    fir, _, _ = out_bytes_case(255, dense(255, seed=53), force_generic=True, expect_path=None, splits_list=([100],), seed=54)
    assert fir.path in ("generic", "lossless64"), fir.path


def test_a_lossy_accumulator_runs_the_exact_order_kernel():
    fir, _, _ = out_bytes_case(63, dense(63), fa=A.Fmt(24, 8, True, "TRN", "WRAP"), fo=fo8_for(63), expect_path=None, splits_list=([5, 300],), seed=52)
    assert fir.path == "generic", fir.path


# 8. chaining: the output tensor of a doubly flagged FIR is the input tensor of a second flagged handle, untouched
def _chain_head(n_ch=3):
    fo_a = A.Fmt(8, 5, True, "RND", "SAT")
    ca = dense(63, seed=80)
    x = rand_raw(np.random.default_rng(81), F8, (n_ch, stream_len(63)))
    ya = oracle_of(63, "SHIFT_REG", F8, FC, FA, fo_a, n_ch).run(ca, x)
    check_share(ya, fo_a, 63, "chain, first stage", want_sat=True)
    a = make(63, ca, fo=fo_a, n_ch=n_ch)
    assert a.path == "mfma_s8"
    mid = a.run(torch.from_numpy(x).to(torch.int8).cuda())
    assert mid.dtype == torch.int8
    same(mid.cpu().numpy().astype(np.int64), ya, "chain, first stage")
    return fo_a, ya, mid


def test_fir_into_fir_on_byte_rows():
    fo_a, ya, mid = _chain_head()
    cb, fo_b = dense(33, seed=82), A.Fmt(16, 9, True, "RND", "SAT")
    yb = oracle_of(33, "SHIFT_REG", fo_a, FC, FA, fo_b, 3).run(cb, ya)
    check_share(yb, fo_b, 33, "chain, second stage")
    b = A.Fir(33, "SHIFT_REG", fo_a, FC, FA, fo_b, n_channels=3, kind="load", in_bytes=True)
    b.set_coeffs(cb)
    assert b.path == "mfma_s8" and b.in_dtype == mid.dtype and b.out_dtype == torch.int16
    same(b.run(mid).cpu().numpy().astype(np.int64), yb, "FIR -> FIR")


def test_fir_into_cic_decimator_on_byte_rows():
    from oracle import OracleCic
    from helpers import ofmt
    fo_a, ya, mid = _chain_head()
    fout = A.Cic(False, 64, 1, 4, fo_a, fo_a, in_bytes=True).int_type
    cic = A.Cic(False, 64, 1, 4, fo_a, fout, n_channels=3, in_bytes=True)
    assert cic.in_dtype == mid.dtype
    yc = OracleCic(False, 64, 1, 4, ofmt(fo_a), ofmt(fout), n_ch=3).run(ya)
    same(cic.run(mid).cpu().numpy().astype(np.int64), yc, "FIR -> CIC decimator")


# 9. supporting behaviour
def test_clone_state_and_run_host():
    n_taps, n_ch = 255, 3
    fo, c = fo8_for(n_taps), dense(n_taps, seed=60)
    rng = np.random.default_rng(61)
    x = [rand_raw(rng, F8, (n_ch, n)) for n in (700, 300, 1100)]
    orc = oracle_of(n_taps, "SHIFT_REG", F8, FC, FA, fo, n_ch)
    want = [orc.run(c, xi) for xi in x]
    check_share(want[0], fo, n_taps, "state, first call")
    both, only_in = make(n_taps, c), make(n_taps, c, out_bytes=False)
    same(run_out_bytes(both, x[0]), want[0], "first call")
    same(run_bytes(only_in, x[0]), want[0], "first call, input flag only")
    blob = both.state()
    assert blob == only_in.state(), "the state blob holds input history only"
    cl = both.clone()
    assert cl.path == "mfma_s8" and cl.out_dtype == torch.int8 and A._lib.lib.acdsp_fir_out_elem_bytes(cl._h) == 1
    into_in, into_both = make(n_taps, c, out_bytes=False), make(n_taps, c)
    into_in.set_state(blob)                                   # a doubly flagged handle's state in an input-flagged twin ...
    same(run_bytes(into_in, x[1]), want[1], "state of both flags in an input-flagged handle")
    into_both.set_state(into_in.state())                      # ... and back
    same(run_out_bytes(into_both, x[2]), want[2], "and back")
    same(run_out_bytes(cl, x[1], [17]), want[1], "clone")
    same(run_out_bytes(both, x[1]), want[1], "the cloned handle goes on")
    same(run_out_bytes(cl, x[2]), want[2], "clone, third call")
    host = make(n_taps, c)
    yh = host.run_host(x[0])
    assert yh.dtype == np.int8 and yh.shape == want[0].shape
    same(yh.astype(np.int64), want[0], "run_host")
    hu = make(n_taps, dense(n_taps, 4), fin=A.Fmt(8, 3, False), fo=A.Fmt(8, 8, False, "RND", "SAT"))
    xu = rand_raw(rng, A.Fmt(8, 3, False), (n_ch, 1500))
    yu = hu.run_host(xu)
    assert yu.dtype == np.uint8
    same(yu.astype(np.int64), oracle_of(n_taps, "SHIFT_REG", A.Fmt(8, 3, False), FC, FA, A.Fmt(8, 8, False, "RND", "SAT"), n_ch).run(dense(n_taps, 4), xu), "run_host, unsigned")


@pytest.mark.parametrize("devices", [[0], [0, 0, 0]])
def test_node_layer_shards_byte_rows_both_ways(devices):
    n_taps, n_ch = 255, 7
    c, fo = dense(n_taps, seed=21), fo8_for(n_taps)
    rng = np.random.default_rng(22)
    node = A.NodeFir(n_taps, "SHIFT_REG", F8, FC, FA, fo, n_ch, devices, kind="load", in_bytes=True, out_bytes=True)
    node.set_coeffs(c)
    assert node.out_dtype == torch.int8
    orc = oracle_of(n_taps, "SHIFT_REG", F8, FC, FA, fo, n_ch)
    for n in (1300, 1024):
        x = rand_raw(rng, F8, (n_ch, n))
        xs = [torch.from_numpy(x[lo:hi].copy()).to(torch.int8).cuda() for lo, hi in node.slices]
        ys = node.run(xs)
        torch.cuda.synchronize()
        assert all(y.dtype == torch.int8 for y in ys)
        want = orc.run(c, x)
        check_share(want, fo, n_taps if n == 1300 else 0, "node call of %d samples" % n)
        same(np.concatenate([y.cpu().numpy().astype(np.int64) for y in ys]), want, "node call of %d samples" % n)
    x = rand_raw(rng, F8, (n_ch, 777))
    yh = node.run_host(x)
    assert yh.dtype == np.int8
    same(yh.astype(np.int64), orc.run(c, x), "node run_host")
    node.close()


def test_calls_replayed_from_a_graph_continue_the_stream():
    n_taps, nch, cs, nk = 255, 8, 4096, 3                     # whole pairs: the branch-free instantiation alone
    c, fo = dense(n_taps, seed=23), fo8_for(n_taps)
    rng = np.random.default_rng(24)
    x = torch.from_numpy(rng.integers(-128, 128, size=(nk, nch, cs), dtype=np.int8)).cuda()
    y0 = make(n_taps, c, n_ch=nch).run(x[0]).cpu().numpy().astype(np.int64)
    want = oracle_of(n_taps, "SHIFT_REG", F8, FC, FA, fo, nch).run(c, x[0].cpu().numpy().astype(np.int64))
    check_share(want, fo, n_taps, "graph, eager call")
    same(y0, want, "eager call")
    _capture_and_check(lambda: make(n_taps, c, n_ch=nch), x, (nch, cs), torch.int8)
