"""GPU parity tests, ac_poly_dec on byte samples (ACDSP_FLAG_IN_BYTES, PolyDec(in_bytes=True)): IN_TYPE of up to 8 bits in 1-byte containers,
one sample plane on the matrix cores.  The HIP engine against the CPU oracle, bit for bit over the whole stream, for the three kernel
families a flagged handle resolves to -- the byte rows of the ring kernel (fir_gen_ring_s8.hip), the window-per-step kernel
(fir_gen_kernel<int8_t, 1, .>) and the long byte kernel (polydec_s8.hip) -- and the exact-order kernel behind them.

Signed samples are <8,2> into ACC <40,20> (F = 6 + 14: exact), unsigned ones <8,0,unsigned> into ACC <48,26>; coefficients are dense
integers(-32768, 32640) of <16,2>.  Every case keeps the guard of test_polydec_long_gpu.py: the oracle's saturated share past the first NTAPS
outputs is at most 20 %.  The path is asserted after every call."""
import numpy as np
import pytest
import torch

import ac_dsp_amd as A
from ac_dsp_amd._lib import lib, PATHS
from oracle import OraclePolyDec
from helpers import ofmt, windowed_sinc, rand_fmt, GraphCase, graph_replays_match_oracle
from test_graph_paths_gpu import chunks_of
from test_polydec_long_gpu import dense, assert_sat_share, same, sinc_set

pytestmark = pytest.mark.gpu

F8 = A.Fmt(8, 2)
F8U = A.Fmt(8, 0, False)
FC = A.Fmt(16, 2)
FA = A.Fmt(40, 20)                          # F = 20 = 6 + 14: exact products
FAU = A.Fmt(48, 26)                         # F = 22 = 8 + 14
FO = A.Fmt(16, 10, True, "RND", "SAT")

# the byte rows of the ring kernel: id -> (DF, OEB, NBT, SPW); ACDSP_RING_S8_ROWS of fir_gen_kernels.hpp
RING_ROWS = {50: (2, 2, 2, 16), 51: (2, 8, 2, 16), 52: (4, 2, 3, 8), 53: (4, 8, 3, 8),
             54: (8, 2, 4, 4), 55: (8, 8, 4, 4), 56: (16, 2, 8, 2), 57: (16, 8, 8, 2)}
FO8 = A.Fmt(40, 20)                         # 8-byte containers


def plan_blocks(nt, df):
    """K-blocks of the ring plan of (NTAPS, DF): fir_gen_window with first = DF - 1"""
    n = nt * df
    a = (((df - 1) % 16) - (n - 1)) % 16
    return (n - 1 + a + 15 * df + 1 + 63) // 64


def largest_ntaps(df, nbt):
    nt = 1
    while plan_blocks(nt + 1, df) <= nbt:
        nt += 1
    return nt


def byte_dtype(fin):
    return torch.int8 if fin.S else torch.uint8


def np_bytes(x, fin):
    return np.ascontiguousarray(x).astype(np.int8 if fin.S else np.uint8)


def dev_bytes(x, fin, off=0):
    """raw words [n_ch][n] -> device rows of 1-byte containers, 16-byte aligned with a stride of a multiple of 16 (off = 0) or `off` bytes off"""
    n_ch, n = x.shape
    stride = (n + 15) // 16 * 16 + 16
    flat = torch.zeros(n_ch * stride + 16, dtype=byte_dtype(fin), device="cuda")
    rows = flat[off:off + n_ch * stride].view(n_ch, stride)[:, :n]
    assert rows.data_ptr() % 16 == off
    rows.copy_(torch.from_numpy(np_bytes(x, fin)).cuda())
    return rows


def run_groups(eng, x, splits=(), expect_path="mfma_gen", ring=None, off=0):
    """x: [n_ch][groups * DF] raw words -> raw outputs; one call per piece between the split points (in output groups); the path after every
    call.  ring = (id, outputs per chunk): a call of at least one whole chunk must report the row's id, a shorter one 0"""
    n_groups = x.shape[1] // eng.df
    bounds = sorted(set([0, n_groups] + [s for s in splits if 0 < s < n_groups]))
    outs, seen = [], set()
    for a, b in zip(bounds[:-1], bounds[1:]):
        # (output rows on 16-byte boundaries: what the ring rows and the window kernel's vector stores take)
        out = torch.empty((x.shape[0], (b - a + 63) // 64 * 64), dtype=A.torch_dtype_for(eng.fout), device="cuda")
        outs.append(eng.run(dev_bytes(x[:, a * eng.df:b * eng.df], eng.fin, off), out=out).cpu().numpy().astype(np.int64))
        assert eng.path == expect_path, (eng.path, expect_path, (a, b))
        if ring is not None:
            want = ring[0] if b - a >= ring[1] else 0
            assert eng.ring_shape == want, (eng.ring_shape, want, (a, b))
            seen.add(eng.ring_shape)
    if ring is not None:
        assert ring[0] in seen, (ring, seen)
    return np.concatenate(outs, axis=1)


def make(nt, df, fin, fa, fo, coeffs, n_ch, **kw):
    kw.setdefault("in_bytes", True)
    eng = A.PolyDec(nt, df, fin, FC, fa, fo, n_channels=n_ch, **kw)
    eng.set_coeffs(coeffs)
    if kw["in_bytes"]:
        assert eng.in_dtype == byte_dtype(fin) and lib.acdsp_polydec_in_elem_bytes(eng._h) == 1
    return eng


def oracle_stream(nt, df, fin, fa, fo, coeffs, x, what=""):
    yo = OraclePolyDec(nt, df, ofmt(fin), ofmt(FC), ofmt(fa), ofmt(fo), n_ch=x.shape[0]).run(coeffs, x)
    assert_sat_share(yo, fo, nt, "%s %d x %d" % (what, nt, df))
    return yo


def case(nt, df, fin=F8, fa=FA, fo=FO, n_ch=3, groups=None, splits_list=((),), seed=0, expect_path="mfma_gen", ring=None, coeffs=None, off=0, x=None):
    """one oracle run, one engine stream per call pattern; returns (last engine handle, x, oracle stream, coefficients)"""
    c = dense(nt * df, seed=seed + 1) if coeffs is None else coeffs
    if groups is None:
        groups = nt + 2 * 1024 + 77
    if x is None:
        x = rand_fmt(np.random.default_rng(seed), fin, (n_ch, groups * df))
    yo = oracle_stream(nt, df, fin, fa, fo, c, x)
    eng = None
    for splits in splits_list:
        eng = make(nt, df, fin, fa, fo, c, n_ch)
        same(run_groups(eng, x, splits, expect_path, ring, off), yo, "%d x %d, splits %s" % (nt, df, list(splits)))
    return eng, x, yo, c


# 1. every compiled byte row of the ring kernel, at one tap per phase and at the largest NTAPS its K-blocks plan
@pytest.mark.parametrize("rid", sorted(RING_ROWS))
@pytest.mark.parametrize("edge", ["one_tap", "largest"])
def test_ring_rows(rid, edge):
    df, oeb, nbt, spw = RING_ROWS[rid]
    nt = 1 if edge == "one_tap" else largest_ntaps(df, nbt)
    assert plan_blocks(nt, df) <= nbt and (edge == "one_tap" or plan_blocks(nt + 1, df) > nbt)
    chunk = spw * 256
    groups = 2 * chunk + 77
    # one call; then ragged calls: after one group, inside a chunk at a group count that is no multiple of 16
    case(nt, df, fo=FO if oeb == 2 else FO8, groups=groups, seed=rid, ring=(rid, chunk), splits_list=([], [1, 1 + chunk + 37]))


# 2. the window-per-step kernel: odd factors, the largest factor it plans (DF = 32: eight K-blocks, eight slots per lane), and 4-byte outputs
# on a ring shape.  (2, 64) stands here as the issue lists it, but no plan of DF = 64 exists -- 15 DF slots alone are 15 K-blocks against
# the eight of fir_gen_window -- so the unflagged handle runs the long kernel there, and the flagged one, which must resolve as the
# unflagged one does, the long byte kernel: the words are checked all the same, the path is the one the unflagged dispatch gives.
@pytest.mark.parametrize("nt,df,fo,path", [(3, 5, FO, "mfma_gen"), (5, 3, FO, "mfma_gen"), (4, 7, FO, "mfma_gen"), (1, 32, FO, "mfma_gen"),
                                           (2, 64, FO, "mfma_s8"), (16, 8, A.Fmt(20, 10, True, "RND", "SAT"), "mfma_gen")])
def test_window_per_step_kernel(nt, df, fo, path):
    assert (plan_blocks(nt, df) <= 8) == (path == "mfma_gen")
    case(nt, df, fo=fo, seed=100 + nt * df, expect_path=path, ring=(0, 0), splits_list=([], [1, 300, 1337]))
    if path != "mfma_gen":
        plain = A.PolyDec(nt, df, F8, FC, FA, fo, n_channels=1)
        plain.set_coeffs(dense(nt * df))
        plain.run(torch.zeros((1, 64 * df), dtype=torch.int16, device="cuda"))
        assert plain.path == "mfma_long", plain.path


# 3. the long byte kernel at the segment edges of test_polydec_long_gpu.py
@pytest.mark.parametrize("nt,df", [
    (16, 32),      # nb 2
    (33, 16),      # the last nb = 2
    (34, 16),      # nb 3
    (481, 2),      # nb 16: one full segment
    (482, 3),      # nb 17: a second segment of one block; odd DF
    (1100, 1),     # DF = 1
    (64, 256),     # the largest DF
    (1024, 16),    # 16384 taps
])
def test_long_byte_kernel_shapes_and_segment_edges(nt, df):
    n_ch = 2 if nt * df == 16384 and df == 16 else 3
    groups = nt + (1024 if df == 256 else 2 * 1024) + 77
    case(nt, df, n_ch=n_ch, groups=groups, seed=200 + nt + df, expect_path="mfma_s8", splits_list=([5, 1040, nt + 600], []))


def test_long_byte_kernel_rows_one_byte_off_alignment():
    case(34, 16, seed=300, expect_path="mfma_s8", splits_list=([700],), off=1)


def test_long_byte_kernel_seventy_channels():
    case(16, 32, n_ch=70, groups=16 + 1024 + 77, seed=301, expect_path="mfma_s8", splits_list=([700],))


def test_long_byte_kernel_slabs_and_groups_under_a_small_scratch_cap():
    nt, df, n_ch = 16, 32, 17
    c = dense(nt * df, seed=4)
    x = rand_fmt(np.random.default_rng(5), F8, (n_ch, (nt + 2 * 1024 + 77) * df))
    yo = oracle_stream(nt, df, F8, FA, FO, c, x)
    per_channel = df * (32 + 1024)                          # bytes of the phase rows of one channel at a slab of 1024 outputs (H = 32)
    for splits in ([], [1000, 1100]):
        eng = make(nt, df, F8, FA, FO, c, n_ch)
        assert eng.long_geometry()[1] == n_ch               # default cap: one group
        eng.set_scratch_cap(8 * per_channel)
        assert eng.long_geometry() == (1024, 8, 8 * per_channel), eng.long_geometry()
        same(run_groups(eng, x, splits, "mfma_s8"), yo, "three groups x slabs of 1024, splits %s" % splits)


# 4. unsigned samples on one shape of each family; narrow types in byte containers
@pytest.mark.parametrize("nt,df,path,ring", [(16, 8, "mfma_gen", (54, 1024)), (3, 5, "mfma_gen", (0, 0)), (16, 32, "mfma_s8", None)])
def test_unsigned_samples(nt, df, path, ring):
    case(nt, df, fin=F8U, fa=FAU, seed=400 + df, expect_path=path, ring=ring, splits_list=([], [1, 1500]))


@pytest.mark.parametrize("fin,fa", [(A.Fmt(5, 1), FA), (A.Fmt(3, 0, False), FAU)])
def test_narrow_types_in_byte_containers(fin, fa):
    case(16, 8, fin=fin, fa=fa, fo=A.Fmt(16, 8, True, "RND", "SAT"), seed=410 + fin.W, ring=(54, 1024), splits_list=([], [777]))


# 5. a flagged handle against an unflagged one on the same values in int16 rows: same words, same family
@pytest.mark.parametrize("nt,df,flagged_path,unflagged_path", [(16, 8, "mfma_gen", "mfma_gen"), (3, 5, "mfma_gen", "mfma_gen"), (16, 32, "mfma_s8", "mfma_long")])
def test_flagged_against_unflagged(nt, df, flagged_path, unflagged_path):
    eng, x, yo, c = case(nt, df, seed=500 + df, expect_path=flagged_path, splits_list=([900],))
    plain = make(nt, df, F8, FA, FO, c, 3, in_bytes=False)
    assert plain.in_dtype == torch.int16 and lib.acdsp_polydec_in_elem_bytes(plain._h) == 2
    outs = []
    for a, b in ((0, 900), (900, x.shape[1] // df)):
        buf = torch.zeros((3, ((b - a) * df + 63) // 64 * 64 + 64), dtype=torch.int16, device="cuda")   # rows on 16-byte boundaries
        buf[:, :(b - a) * df] = torch.from_numpy(x[:, a * df:b * df].copy()).to(torch.int16)
        outs.append(plain.run(buf[:, :(b - a) * df]).cpu().numpy().astype(np.int64))
        assert plain.path == unflagged_path, plain.path
    same(np.concatenate(outs, axis=1), yo, "unflagged twin")


# 6. output conversion at 16 x 8
@pytest.mark.parametrize("fo", [
    A.Fmt(12, 6, True, "RND", "SAT"),                       # the clamp acts: 2.6 % of the outputs
    A.Fmt(18, 2, True, "TRN", "WRAP"),                      # 4-byte containers: the window-per-step kernel
    A.Fmt(40, 20),                                          # 8-byte containers
    A.Fmt(24, 12, True, "RND_CONV", "SAT_SYM"),             # outside the branch-free conversion
])
def test_output_conversion_at_16_x_8(fo):
    case(16, 8, fo=fo, seed=600 + fo.W, splits_list=([], [1100]))


# 7. saturating accumulators
def test_a_saturating_accumulator_no_partial_sum_can_reach_stays_on_the_matrix_cores():
    c = sinc_set(16, 8, FC)
    case(16, 8, fa=A.Fmt(40, 20, True, "TRN", "SAT"), seed=700, coeffs=c, ring=(54, 1024), splits_list=([], [500]))


def test_a_saturating_accumulator_that_can_be_reached_runs_the_exact_order_kernel():
    case(16, 8, fa=A.Fmt(28, 8, True, "TRN", "SAT"), seed=701, expect_path="generic", splits_list=([], [500]))


# 8. state
def test_blobs_move_between_a_matrix_core_handle_and_an_exact_order_one():
    for nt, df, path in ((16, 8, "mfma_gen"), (16, 32, "mfma_s8")):
        c = dense(nt * df, seed=800)
        n_ch, g = 3, 1200
        x = rand_fmt(np.random.default_rng(801), F8, (n_ch, 3 * g * df))
        yo = oracle_stream(nt, df, F8, FA, FO, c, x)
        fast, slow = make(nt, df, F8, FA, FO, c, n_ch), make(nt, df, F8, FA, FO, c, n_ch, force_generic=True)
        y0 = run_groups(fast, x[:, :g * df], (), path)
        slow.set_state(fast.state())
        y1 = run_groups(slow, x[:, g * df:2 * g * df], (), "generic")
        fresh = make(nt, df, F8, FA, FO, c, n_ch)
        fresh.set_state(slow.state())
        y2 = run_groups(fresh, x[:, 2 * g * df:], (), path)
        same(np.concatenate([y0, y1, y2], axis=1), yo, "%d x %d: matrix cores -> exact order -> matrix cores" % (nt, df))


def test_flagged_and_unflagged_blobs_refuse_each_other_and_clone_and_reset():
    nt, df, n_ch, g = 16, 8, 3, 1100
    c = dense(nt * df, seed=810)
    x = rand_fmt(np.random.default_rng(811), F8, (n_ch, 2 * g * df))
    yo = oracle_stream(nt, df, F8, FA, FO, c, x)
    flagged, plain = make(nt, df, F8, FA, FO, c, n_ch), make(nt, df, F8, FA, FO, c, n_ch, in_bytes=False)
    y0 = run_groups(flagged, x[:, :g * df])
    xd16 = torch.zeros((n_ch, (g * df + 63) // 64 * 64 + 64), dtype=torch.int16, device="cuda")
    xd16[:, :g * df] = torch.from_numpy(x[:, :g * df].copy()).to(torch.int16)
    same(plain.run(xd16[:, :g * df]).cpu().numpy().astype(np.int64), yo[:, :g], "unflagged, first call")
    assert len(flagged.state()) < len(plain.state())
    for dst, src in ((plain, flagged), (flagged, plain)):
        with pytest.raises(A.AcdspError) as e:
            dst.set_state(src.state())
        assert e.value.code == 1, e.value                   # ACDSP_EINVAL
    cl = flagged.clone()
    assert cl.in_bytes and cl.in_dtype == torch.int8
    same(np.concatenate([y0, run_groups(flagged, x[:, g * df:])], axis=1), yo, "after the refused blob")
    same(np.concatenate([y0, run_groups(cl, x[:, g * df:])], axis=1), yo, "clone")
    xd16[:, :g * df] = torch.from_numpy(x[:, g * df:].copy()).to(torch.int16)
    same(plain.run(xd16[:, :g * df]).cpu().numpy().astype(np.int64), yo[:, g:], "unflagged after the refused blob")
    flagged.reset()
    same(run_groups(flagged, x[:, :g * df]), yo[:, :g], "after reset()")


def test_rows_off_alignment_on_a_ring_shape_run_the_exact_order_kernel_and_rejoin():
    nt, df, n_ch = 16, 8, 3
    c = dense(nt * df, seed=820)
    x = rand_fmt(np.random.default_rng(821), F8, (n_ch, 3 * 1100 * df))
    yo = oracle_stream(nt, df, F8, FA, FO, c, x)
    eng = make(nt, df, F8, FA, FO, c, n_ch)
    n = 1100 * df
    y = [run_groups(eng, x[:, :n], ring=(54, 1024)), run_groups(eng, x[:, n:2 * n], expect_path="generic", off=1),
         run_groups(eng, x[:, 2 * n:], ring=(54, 1024))]
    same(np.concatenate(y, axis=1), yo, "aligned, 1 byte off, aligned")


# 9. other call routes
@pytest.mark.parametrize("nt,df", [(16, 8), (3, 5), (16, 32)])
def test_run_host_equals_run(nt, df):
    c = dense(nt * df, seed=900)
    x = rand_fmt(np.random.default_rng(901), F8, (3, 1300 * df))
    yo = oracle_stream(nt, df, F8, FA, FO, c, x)
    eng = make(nt, df, F8, FA, FO, c, 3)
    y = [eng.run_host(np_bytes(x[:, :700 * df], F8)), eng.run_host(np_bytes(x[:, 700 * df:], F8))]
    same(np.concatenate(y, axis=1).astype(np.int64), yo, "run_host")


@pytest.mark.parametrize("shards", [1, 3, 8])
def test_node_layer_shards_byte_rows(shards):
    nt, df, n_ch = 16, 8, 9
    c = dense(nt * df, seed=910)
    node = A.NodePolyDec(nt, df, F8, FC, FA, FO, n_ch, [0] * shards, in_bytes=True)
    node.set_coeffs(c)
    orc = OraclePolyDec(nt, df, ofmt(F8), ofmt(FC), ofmt(FA), ofmt(FO), n_ch=n_ch)
    rng = np.random.default_rng(911)
    stream = []
    for groups in (1300, 1024):
        x = rand_fmt(rng, F8, (n_ch, groups * df))
        xs = [dev_bytes(x[lo:hi], F8) for lo, hi in node.slices]
        ys = node.run(xs)
        torch.cuda.synchronize()
        stream.append(orc.run(c, x))
        same(np.concatenate([y.cpu().numpy().astype(np.int64) for y in ys]), stream[-1], "node call of %d groups" % groups)
        handles = [node.shard_handle(s) for s in range(len(node.slices))]
        assert [PATHS[lib.acdsp_polydec_path(h)] for h in handles] == ["mfma_gen"] * shards
        assert [lib.acdsp_polydec_in_elem_bytes(h) for h in handles] == [1] * shards
    assert_sat_share(np.concatenate(stream, axis=1), FO, nt, "node stream")
    node.close()


@pytest.mark.parametrize("nt,df,path,n", [(16, 8, "mfma_gen", 1100 * 8), (3, 5, "mfma_gen", 1104 * 5), (16, 32, "mfma_s8", 1100 * 32)])
def test_calls_replayed_from_a_graph_continue_the_stream(nt, df, path, n):
    n_ch = 3
    c = dense(nt * df, seed=920)
    streams = []

    def oracle():
        o = OraclePolyDec(nt, df, ofmt(F8), ofmt(FC), ofmt(FA), ofmt(FO), n_ch=n_ch)
        streams.append([])

        def run(x, out=streams[-1]):
            out.append(o.run(c, x))
            return out[-1]
        return run

    # the helper hands over rows of IN_TYPE's plain containers (int16): the conversion to byte rows is part of the captured call.  Every
    # length is a multiple of 16, so the contiguous byte rows are 16-byte aligned
    gcase = GraphCase(lambda: make(nt, df, F8, FA, FO, c, n_ch), lambda e, xd: e.run(xd.to(torch.int8)), oracle, F8, lambda e: e.path)
    assert n % 16 == 0
    rng = np.random.default_rng(921)
    graph_replays_match_oracle(gcase, [rand_fmt(rng, F8, (n_ch, 320 * df))], chunks_of(922, F8, n_ch, [n]), rand_fmt(rng, F8, (n_ch, 80 * df)), path)
    assert streams and all(len(s) > 0 for s in streams)
    for s in streams:
        assert_sat_share(np.concatenate(s, axis=1), FO, nt, "graph stream")
