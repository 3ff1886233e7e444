"""GPU parity tests, ac_intg_dump on 1-byte input containers (ACDSP_FLAG_IN_BYTES, IntgDump(in_bytes=True)): the selection-matrix kernel on one
sample plane (path "mfma"), the LDS-tiled kernel on byte rows, and the exact-order kernel, everything bit for bit against OracleIntgDump
(reference include/ac_dsp/ac_intg_dump.h:93-147)."""
import ctypes as C

import numpy as np
import pytest
import torch

import ac_dsp_amd as A
from ac_dsp_amd import _lib as L
from oracle import OracleIntgDump
from helpers import ofmt, rand_fmt

pytestmark = pytest.mark.gpu

S84 = A.Fmt(8, 4)                      # signed, F = 4
U88 = A.Fmt(8, 8, False)               # unsigned, F = 0
A32 = A.Fmt(32, 16)                    # ACC = OUT of the bench row: acc.F - in.F = 12 on <8,4>


def byte_dtype(fin):
    return torch.int8 if fin.S else torch.uint8


def dev_bytes(x, fin, off=0):
    """[rows][n] raw words -> device rows of 1-byte containers; row 0 starts `off` bytes behind a 16-byte boundary and the pitch is a multiple
    of 16 bytes, so off = 0 is the layout the fast kernel takes and off = 1 one it has to decline"""
    x = np.atleast_2d(x)
    n = x.shape[1]
    buf = torch.zeros((x.shape[0], (n + off + 15) // 16 * 16 + 16), dtype=byte_dtype(fin), device="cuda")
    view = buf[:, off:off + n]
    view.copy_(torch.from_numpy(np.ascontiguousarray(x).astype(np.int8 if fin.S else np.uint8)))
    return view


def make(ns, chn, fin, fa, fo, n_obj, in_bytes=True):
    return A.IntgDump(ns, chn, fin, fa, fo, n_objects=n_obj, in_bytes=in_bytes), OracleIntgDump(ns, chn, ofmt(fin), ofmt(fa), ofmt(fo), n_obj=n_obj)


def same(y, yo, what=""):
    y = y.cpu().numpy().astype(np.int64) if torch.is_tensor(y) else np.asarray(y).astype(np.int64)
    assert y.shape == yo.shape, (what, y.shape, yo.shape)
    bad = np.argwhere(y != yo)
    assert bad.size == 0, "%s: %d words differ from the oracle, first at %s: %d != %d" % (what, len(bad), bad[0], y[tuple(bad[0])], yo[tuple(bad[0])])


def full_scale_rows(x, fin):
    lo, hi = (-(1 << (fin.W - 1)), (1 << (fin.W - 1)) - 1) if fin.S else (0, (1 << fin.W) - 1)
    x[0], x[1] = hi, lo
    return x


def check_calls(ns, chn, fin, fa, fo, calls, paths, n_obj=5, seed=0, off=0):
    rng = np.random.default_rng(seed)
    eng, orc = make(ns, chn, fin, fa, fo, n_obj)
    for n_sample, path in zip(calls, paths):
        ni, no = eng.counts(n_sample)
        x = full_scale_rows(rand_fmt(rng, fin, (n_obj, ni)), fin)
        y = eng.run(dev_bytes(x, fin, off), n_sample)
        assert eng.path == path, (eng.path, path)
        same(y, orc.run(x, n_sample), "CHN %d, %d blocks" % (chn, len(n_sample)))
    return eng


# 1. the fast kernel, two calls each
FAST = [
    # chn, rounds, n_blk, IN, ACC, OUT
    (4, 64, 96, S84, A32, A32),                                                             # the bench block; acc.F - in.F = 12
    (1, 16, 256, U88, A.Fmt(24, 24, False), A.Fmt(24, 24, False)),                          # one partial segment per block; acc.F - in.F = 0
    (3, 16, 37, A.Fmt(7, 7, False), A.Fmt(20, 20, False), A.Fmt(20, 20, False)),            # 48-sample blocks, a ragged last tile
    (5, 64, 33, A.Fmt(1, 1, False), A.Fmt(16, 16, False), A.Fmt(16, 16, False)),            # selection-fragment period P = 5
    (7, 48, 20, A.Fmt(6, 2), A.Fmt(48, 13), A.Fmt(48, 13)),                                 # the last segment a quarter full; acc.F - in.F = 31
    (12, 100, 19, S84, A32, A32),
    (16, 2, 130, U88, A.Fmt(20, 20, False), A.Fmt(20, 20, False)),                          # two loads per block
    (2, 1000, 9, S84, A.Fmt(27, 11), A.Fmt(20, 6, True, "RND", "SAT")),                     # 31.25 segments
    (8, 4096, 17, A.Fmt(8, 1), A.Fmt(30, 23), A.Fmt(30, 23)),                               # blocks of 32 KB; acc.F - in.F = 0
    # blocks of 16 and 32 bytes with at least 4 rounds: 4 / 2 blocks share a 64-byte column; block counts that leave a column part empty
    (4, 4, 131, S84, A32, A32),                                                             # 4 blocks x 4 channels = 16 rows
    (2, 16, 37, U88, A.Fmt(24, 24, False), A.Fmt(12, 12, False, "TRN", "SAT")),
    (8, 4, 51, S84, A32, A32),                                                              # 2 blocks x 8 channels = 16 rows
    (2, 8, 70, A.Fmt(5, 5, False), A.Fmt(16, 14, False), A.Fmt(16, 14, False)),
    (16, 1, 40, S84, A32, A32),                                                             # fewer than 4 rounds: a column per block
]


@pytest.mark.parametrize("chn,rounds,n_blk,fin,fa,fo", FAST)
def test_fast_kernel_shapes(chn, rounds, n_blk, fin, fa, fo):
    check_calls(rounds, chn, fin, fa, fo, [[rounds] * n_blk, [rounds] * (n_blk // 2)], ["mfma", "mfma"], seed=100 * chn + rounds)


# 2. full scale
@pytest.mark.parametrize("fin,fa", [(S84, A32), (U88, A.Fmt(32, 28, False))])
def test_full_scale_rows_and_a_block_count_that_is_no_multiple_of_16(fin, fa):
    chn, rounds, n_blk, n_obj = 4, 64, 37, 5
    lo, hi = (-128, 127) if fin.S else (0, 255)
    eng, orc = make(rounds, chn, fin, fa, fa, n_obj)
    n = chn * rounds * n_blk
    x = np.empty((n_obj, n), dtype=np.int64)
    x[0], x[1] = lo, hi                                     # every sample -128 / 127 (0 / 255)
    x[2, 0::2], x[2, 1::2] = lo, hi                         # alternating extremes: channels 0, 2 at one rail and 1, 3 at the other
    x[3, 0::2], x[3, 1::2] = hi, lo
    x[4] = np.where((np.arange(n) // chn) % 2 == 0, lo, hi)  # alternating round by round
    y = eng.run(dev_bytes(x, fin), [rounds] * n_blk)
    assert eng.path == "mfma"
    same(y, orc.run(x, [rounds] * n_blk))


@pytest.mark.parametrize("fin,fa", [(S84, A.Fmt(32, 28)), (U88, A.Fmt(32, 32, False))])
def test_int32_plane_sums_far_up(fin, fa):
    # 2^16 rounds of full-scale bytes: |sum| = 2^23 per block on the re-biased plane as well
    chn, rounds, n_blk, n_obj = 1, 1 << 16, 16, 3
    lo, hi = (-128, 127) if fin.S else (0, 255)
    eng, orc = make(rounds, chn, fin, fa, fa, n_obj)
    x = rand_fmt(np.random.default_rng(5), fin, (n_obj, rounds * n_blk))
    x[0], x[1] = lo, hi
    y = eng.run(dev_bytes(x, fin), [rounds] * n_blk)
    assert eng.path == "mfma"
    same(y, orc.run(x, [rounds] * n_blk))


# 3. OUT_TYPE conversion on the byte path: the sets of the CIC byte tests (RND_CONV / SAT_SYM and TRN_ZERO / SAT_ZERO take the general requant)
@pytest.mark.parametrize("q,o,wo,io", [("RND", "SAT", 12, 4), ("RND", "SAT", 20, 4), ("TRN", "WRAP", 18, 2), ("RND_CONV", "SAT_SYM", 24, 12),
                                       ("TRN_ZERO", "SAT_ZERO", 40, 40)])
def test_output_type_conversion_on_the_byte_path(q, o, wo, io):
    check_calls(64, 4, S84, A32, A.Fmt(wo, io, True, q, o), [[64] * 96, [64] * 48], ["mfma", "mfma"], seed=wo)


# 4. saturating ACC_TYPE
def test_a_saturating_accumulator_that_cannot_saturate_stays_on_the_fast_kernel():
    # 64 rounds x 128 x 2^8 = 2^21 < 2^23
    fa = A.Fmt(24, 12, True, "TRN", "SAT")
    check_calls(64, 4, S84, fa, A.Fmt(24, 12), [[64] * 96, [64] * 48], ["mfma", "mfma"], seed=41)


def test_a_saturating_accumulator_that_full_scale_drives_into_the_rails_runs_in_exact_order():
    # 2^21 against the 2^17 of <18,6>: rows 0 and 1 (full scale) sit on the rails
    fa = A.Fmt(18, 6, True, "TRN", "SAT")
    check_calls(64, 4, S84, fa, A.Fmt(18, 6), [[64] * 96, [64] * 48], ["exact_order", "exact_order"], seed=42)


# 5. declines, each still exact
def test_blocks_that_carry_sums_run_in_exact_order():
    # non-uniform n_sample with a block that does not dump (100 > NS: NS rounds, the sums go on into the next block)
    check_calls(64, 4, S84, A32, A32, [[64, 64, 3, 100, 64, 7]], ["exact_order"], seed=51)


def test_non_uniform_blocks_that_all_dump_take_the_tiled_kernel():
    # the launcher's rule for every container: nothing carried and every block dumps -> LDS-tiled kernel, whatever the rounds per block
    check_calls(64, 4, S84, A32, A32, [[64, 64, 3, 64, 17]], ["tile"], seed=52)


def test_a_block_of_15_samples_takes_the_tiled_kernel():
    check_calls(5, 3, S84, A32, A32, [[5] * 70, [5] * 35], ["tile", "tile"], seed=53)


def test_rows_one_byte_off_a_16_byte_boundary_take_the_tiled_kernel():
    check_calls(64, 4, S84, A32, A32, [[64] * 40, [64] * 20], ["tile", "tile"], seed=54, off=1)
    check_calls(64, 4, U88, A.Fmt(24, 24, False), A.Fmt(24, 24, False), [[64] * 40], ["tile"], seed=55, off=1)


def test_17_channels_take_the_tiled_kernel_and_300_the_exact_order_kernel():
    check_calls(16, 17, S84, A32, A32, [[16] * 48, [16] * 24], ["tile", "tile"], seed=56)
    check_calls(16, 300, U88, A.Fmt(24, 24, False), A.Fmt(24, 24, False), [[16] * 6, [16] * 3], ["exact_order", "exact_order"], n_obj=3, seed=57)


def test_pending_sums_and_uniform_calls_alternate_on_every_kernel_family():
    """as the test of this name on int16 rows: calls that leave an undumped sum behind (exact-order kernel, temp[] non-zero), calls that dump it,
    then uniform calls on the kernels that leave temp[] alone, several times round, with full-scale rows so that a stale temp[] would show"""
    ns, chn, n_obj = 64, 4, 5
    rng = np.random.default_rng(21)
    eng, orc = make(ns, chn, S84, A32, A32, n_obj)
    uniform, leaves_pending, dumps_pending, ragged_clean = [ns] * 64, [ns, ns, 7, 0], [ns, ns], [5, ns, 9, ns]
    seen = []
    for n_sample in [uniform, leaves_pending, dumps_pending, uniform, uniform, leaves_pending, leaves_pending, dumps_pending, ragged_clean, uniform,
                     [ns] * 3, leaves_pending, uniform]:
        ni, no = eng.counts(n_sample)
        x = full_scale_rows(rand_fmt(rng, S84, (n_obj, ni)), S84)
        y = eng.run(dev_bytes(x, S84), n_sample)
        seen.append(eng.path)
        same(y, orc.run(x, n_sample), "%s on %s" % (n_sample[:6], eng.path))
    assert seen[0] == "mfma" and seen[1] == "exact_order" and seen[2] == "exact_order" and seen[3] == "mfma" and seen[8] == "tile" and seen[9] == "mfma", seen
    assert seen[-1] == "exact_order", seen                   # the last call starts with a pending sum


# 6. flagged against unflagged
def _pair(ns, chn, fin, fa, fo, n_obj):
    return A.IntgDump(ns, chn, fin, fa, fo, n_objects=n_obj, in_bytes=True), A.IntgDump(ns, chn, fin, fa, fo, n_objects=n_obj)


def _run_both(flagged, plain, x, fin, n_sample):
    yf = flagged.run(dev_bytes(x, fin), n_sample).cpu().numpy().astype(np.int64)
    yp = plain.run(torch.from_numpy(x).to(torch.int16).cuda(), n_sample).cpu().numpy().astype(np.int64)
    return yf, yp


def test_flagged_and_unflagged_handles_agree_and_trade_their_state():
    ns, chn, n_obj = 64, 4, 3
    rng = np.random.default_rng(61)
    flagged, plain = _pair(ns, chn, S84, A32, A32, n_obj)
    orc = OracleIntgDump(ns, chn, ofmt(S84), ofmt(A32), ofmt(A32), n_obj=n_obj)
    assert flagged.in_bytes and flagged.in_dtype == torch.int8 and not plain.in_bytes and plain.in_dtype == torch.int16
    assert L.lib.acdsp_intgdump_in_elem_bytes(flagged._h) == 1 and L.lib.acdsp_intgdump_in_elem_bytes(plain._h) == 2
    calls = [[ns] * 32, [ns, 5, 0], [9, ns, 100]]                         # the second and the third call end on sums that are pending
    xs = [full_scale_rows(rand_fmt(rng, S84, (n_obj, flagged.counts(c)[0])), S84) for c in calls]
    for c, x in zip(calls, xs):
        yf, yp = _run_both(flagged, plain, x, S84, c)
        yo = orc.run(x, c)
        same(yf, yo, "flagged")
        same(yp, yo, "unflagged")
    # sums are pending: the blob of either handle restores into a fresh handle of the other kind, and both go on with the stream
    blob_f, blob_p = flagged.state(), plain.state()
    assert blob_f == blob_p
    flagged2, plain2 = _pair(ns, chn, S84, A32, A32, n_obj)
    plain2.set_state(blob_f)
    flagged2.set_state(blob_p)
    nxt = [7, ns, ns]
    x = rand_fmt(rng, S84, (n_obj, flagged.counts(nxt)[0]))
    yo = orc.run(x, nxt)
    yf, yp = _run_both(flagged2, plain2, x, S84, nxt)
    same(yf, yo, "flagged handle on the unflagged handle's state")
    same(yp, yo, "unflagged handle on the flagged handle's state")
    # clone() mid-stream keeps the flag and continues; the original is untouched by what the clone runs
    twin = flagged.clone()
    assert twin.in_bytes and twin.in_dtype == torch.int8 and L.lib.acdsp_intgdump_in_elem_bytes(twin._h) == 1
    same(twin.run(dev_bytes(x, S84), nxt), yo, "clone")
    same(flagged.run(dev_bytes(x, S84), nxt), yo, "original behind its clone")
    # reset() starts the stream again
    flagged.run(dev_bytes(xs[1], S84), calls[1])                           # leaves sums pending
    flagged.reset()
    fresh = OracleIntgDump(ns, chn, ofmt(S84), ofmt(A32), ofmt(A32), n_obj=n_obj)
    y = flagged.run(dev_bytes(xs[0], S84), calls[0])
    assert flagged.path == "mfma"
    same(y, fresh.run(xs[0], calls[0]), "after reset()")


# 7. run_host equals run
@pytest.mark.parametrize("fin,fa", [(S84, A32), (U88, A.Fmt(24, 24, False))])
def test_run_host_equals_run(fin, fa):
    ns, chn, n_obj = 64, 3, 4
    rng = np.random.default_rng(71)
    host, dev = A.IntgDump(ns, chn, fin, fa, fa, n_objects=n_obj, in_bytes=True), A.IntgDump(ns, chn, fin, fa, fa, n_objects=n_obj, in_bytes=True)
    orc = OracleIntgDump(ns, chn, ofmt(fin), ofmt(fa), ofmt(fa), n_obj=n_obj)
    for n_sample in ([ns] * 20, [ns, 5, 0, 9], [ns] * 10):
        x = full_scale_rows(rand_fmt(rng, fin, (n_obj, host.counts(n_sample)[0])), fin)
        yh = host.run_host(x, n_sample)
        yd = dev.run(dev_bytes(x, fin), n_sample)
        assert host.path == dev.path
        yo = orc.run(x, n_sample)
        same(yh, yo, "run_host")
        same(yd, yo, "run")


# 8. the node layer
def test_node_bank_on_byte_rows():
    ns, chn, n_obj, n_blk = 64, 4, 7, 40
    node = A.NodeIntgDump(ns, chn, S84, A32, A32, n_obj, [0, 0, 0], in_bytes=True)
    assert node.in_bytes and node.in_dtype == torch.int8
    orc = OracleIntgDump(ns, chn, ofmt(S84), ofmt(A32), ofmt(A32), n_obj=n_obj)
    rng = np.random.default_rng(81)
    for n_sample in ([ns] * n_blk, [ns, 3, 0], [ns] * n_blk):
        n = int(sum(s if 1 <= s <= ns else ns for s in n_sample)) * chn
        x = full_scale_rows(rand_fmt(rng, S84, (n_obj, n)), S84)
        ys = node.run([dev_bytes(x[lo:hi], S84) for lo, hi in node.slices], n_sample)
        y = np.concatenate([t.cpu().numpy().astype(np.int64) for t in ys])
        same(y, orc.run(x, n_sample), "node")


# 9. one wave walking more than one tile
def test_a_wave_walks_two_tiles():
    """The launcher gives a wave ceil(16 KB / tile bytes) tiles (a tile = 16 columns; a column = a block, or the 4 / 2 blocks of 16 / 32 bytes
    that share 64 bytes) and halves that while waves x objects stay under 16384.  The smallest tile is 256 bytes: blocks of 16 bytes that do
    not share a column (CHN 16, one round).  64 tiles per wave to start with; 64 objects x 8192 blocks = 512 tiles per object stop the halving
    at 2 tiles per wave (256 waves x 64 objects = 16384), the smallest such product: 8 MiB of samples."""
    chn, rounds, n_obj, n_blk = 16, 1, 64, 8192
    eng, orc = make(rounds, chn, S84, A32, A32, n_obj)
    x = full_scale_rows(rand_fmt(np.random.default_rng(91), S84, (n_obj, chn * rounds * n_blk)), S84)
    y = eng.run(dev_bytes(x, S84), [rounds] * n_blk)
    assert eng.path == "mfma"
    same(y, orc.run(x, [rounds] * n_blk))


def test_a_wave_walks_two_tiles_of_shared_columns():
    # CHN 1, 16 rounds: 4 blocks per column, tiles of 1 KB, 16 per wave to start with; 64 objects x 32768 blocks = 512 tiles per object stop the
    # halving at 2.  Seven blocks more: a tile of its own, its second column three quarters empty
    chn, rounds, n_obj, n_blk = 1, 16, 64, 32768 + 7
    eng, orc = make(rounds, chn, U88, A.Fmt(24, 24, False), A.Fmt(24, 24, False), n_obj)
    x = full_scale_rows(rand_fmt(np.random.default_rng(93), U88, (n_obj, rounds * n_blk)), U88)
    y = eng.run(dev_bytes(x, U88), [rounds] * n_blk)
    assert eng.path == "mfma"
    same(y, orc.run(x, [rounds] * n_blk))


def test_a_wave_walks_two_tiles_of_a_periodic_pattern():
    # the same rule on CHN 3, blocks of 48 bytes (22 tiles per wave to start with, 2 at 518 tiles x 64 objects): fragments from the LDS table,
    # eight tile ends per batch, a ragged last tile
    chn, rounds, n_obj, n_blk = 3, 16, 64, 8192 + 16 * 5 + 3
    eng, orc = make(rounds, chn, S84, A32, A32, n_obj)
    x = full_scale_rows(rand_fmt(np.random.default_rng(92), S84, (n_obj, chn * rounds * n_blk)), S84)
    y = eng.run(dev_bytes(x, S84), [rounds] * n_blk)
    assert eng.path == "mfma"
    same(y, orc.run(x, [rounds] * n_blk))


# 10. graph capture
def test_graph_capture_on_byte_rows():
    ns, chn, n_obj, n_blk = 64, 4, 3, 64
    tbl = np.full(n_blk, ns, dtype=np.int64)
    eng, orc = make(ns, chn, S84, A32, A32, n_obj)
    rng = np.random.default_rng(101)
    n = ns * chn * n_blk
    xs = [full_scale_rows(rand_fmt(rng, S84, (n_obj, n)), S84) for _ in range(4)]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        y0 = eng.run(dev_bytes(xs[0], S84), tbl)              # eager call with the table on the capture stream
    side.synchronize()
    same(y0, orc.run(xs[0], tbl), "eager call in front of the capture")
    xd = dev_bytes(xs[1], S84)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        y = eng.run(xd, tbl)
        path = eng.path
    torch.cuda.synchronize()
    assert path == "mfma"
    for r in range(3):
        xd.copy_(torch.from_numpy(xs[1 + r].astype(np.int8)))
        y.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        same(y, orc.run(xs[1 + r], tbl), "replay %d" % r)


def test_a_captured_call_with_another_table_is_refused():
    ns, chn, n_obj, n_blk = 64, 4, 3, 32
    tbl = np.full(n_blk, ns, dtype=np.int64)
    other = tbl.copy()
    other[3] = ns // 2
    eng, orc = make(ns, chn, S84, A32, A32, n_obj)
    rng = np.random.default_rng(102)
    x0, x1 = rand_fmt(rng, S84, (n_obj, ns * chn * n_blk)), rand_fmt(rng, S84, (n_obj, ns * chn * n_blk))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        eng.run(dev_bytes(x0, S84), tbl)
    side.synchronize()
    orc.run(x0, tbl)
    xd = dev_bytes(x1, S84)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    err = None
    with torch.cuda.graph(g, stream=side):
        y = eng.run(xd, tbl)
        try:
            eng.run(xd, other)
        except A.AcdspError as e:
            err = e
    torch.cuda.synchronize()
    assert err is not None and err.code == 5 and "graph capture" in str(err) and "table differs" in str(err), err   # ACDSP_ESTATE
    y.zero_()
    g.replay()
    torch.cuda.synchronize()
    same(y, orc.run(x1, tbl), "replay of the legal call")


def test_the_raw_abi_reads_byte_rows_under_the_flag():
    # acdsp_intgdump_run on a flagged descriptor, without the Python class: 1-byte rows, in_stride in elements
    ns, chn, n_obj, n_blk = 16, 2, 2, 8
    fa = A.Fmt(24, 24, False)
    d = L.IntgDumpDesc(ns, chn, n_obj, U88, fa, fa, 0, L.FLAG_IN_BYTES)
    h = C.c_void_p()
    L.check(L.lib.acdsp_intgdump_create(C.byref(d), C.byref(h)))
    try:
        x = rand_fmt(np.random.default_rng(111), U88, (n_obj, ns * chn * n_blk))
        xd = dev_bytes(x, U88)
        out = torch.zeros((n_obj, chn * n_blk), dtype=torch.int32, device="cuda")
        tbl = np.full(n_blk, ns, dtype=np.int64)
        n_out = C.c_int64()
        L.check(L.lib.acdsp_intgdump_run(h, C.c_void_p(xd.data_ptr()), xd.stride(0), tbl.ctypes.data_as(C.POINTER(C.c_int64)), n_blk,
                                         C.c_void_p(out.data_ptr()), out.stride(0), C.byref(n_out), None))
        torch.cuda.synchronize()
        assert n_out.value == chn * n_blk and L.lib.acdsp_intgdump_path(h) == 3
        same(out, OracleIntgDump(ns, chn, ofmt(U88), ofmt(fa), ofmt(fa), n_obj=n_obj).run(x, tbl))
    finally:
        L.lib.acdsp_intgdump_destroy(h)
