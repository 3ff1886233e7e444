"""GPU parity tests, long ac_poly_dec prototypes (polydec_long.hip: every exact-sum shape of 16-bit types the ring kernel cannot plan, up to
NTAPS*DF = 16384 and DF = 256): the HIP engine against the CPU oracle, bit for bit over the whole stream.

A case streams NTAPS + 2 * 1024 + 77 output groups (NTAPS + 1024 + 77 at DF = 256, for the oracle's time): every tap of every phase sees data,
and the stream holds two complete 1024-output steps and a ragged one.  Dense full-range sets into OUT <16,10,RND,SAT> saturate well under
1 % of the outputs past the fill; every case asserts that the oracle's saturated share past the first NTAPS outputs is at most 20 %.  The
path is asserted after every call."""
import numpy as np
import pytest
import torch

import ac_dsp_amd as A
from ac_dsp_amd._lib import lib, PATHS
from oracle import OraclePolyDec
from helpers import ofmt, windowed_sinc, rand_fmt, GraphCase, graph_replays_match_oracle
from test_graph_paths_gpu import chunks_of

pytestmark = pytest.mark.gpu

F16 = A.Fmt(16, 2)
FA = A.Fmt(48, 20)                          # F = 28 = F_in + F_coeff: exact products, 19 integer bits of headroom
FO = A.Fmt(16, 10, True, "RND", "SAT")


def stream_groups(nt, df):
    return nt + (1024 if df == 256 else 2 * 1024) + 77


def dense(n, seed=1):
    return np.random.default_rng(seed).integers(-32768, 32640, size=n, dtype=np.int64)


def sinc_set(nt, df, fc=F16):
    """a windowed-sinc prototype of NTAPS*DF taps in the reference's layout c[tp + NTAPS d] = h[d + tp DF]"""
    h = windowed_sinc(nt * df, 0.4 / df, fc)
    return np.array([h[d + tp * df] for d in range(df) for tp in range(nt)], dtype=np.int64)


def sat_share(yo, fo, nt):
    """share of the oracle's outputs past the first NTAPS that sit on a bound of OUT_TYPE"""
    lo = -(1 << (fo.W - 1)) if fo.S else 0
    hi = (1 << (fo.W - 1)) - 1 if fo.S else (1 << fo.W) - 1
    tail = yo[:, nt:]
    return float(np.mean((tail <= lo + 1) | (tail >= hi)))


def assert_sat_share(yo_stream, fo, nt, what):
    """the guard of every case: the oracle's whole stream (calls concatenated) is not mostly clamped outputs"""
    share = sat_share(yo_stream, fo, nt)
    print("%s: saturated share past the fill %.4f" % (what, share))
    assert share <= 0.20, (what, share)


def same(y, yo, what=""):
    assert y.shape == yo.shape, (what, y.shape, yo.shape)
    bad = np.argwhere(y != yo)
    assert bad.size == 0, "%s: %d mismatches, first at %s: got %d want %d" % (what, len(bad), bad[0], y[tuple(bad[0])], yo[tuple(bad[0])])


def run_groups(eng, x, splits=(), expect_path="mfma_long"):
    """x: [n_ch][groups * DF] raw words -> raw outputs; one call per piece between the split points (in output groups); the path after every call"""
    dt = A.torch_dtype_for(eng.fin)
    n_groups = x.shape[1] // eng.df
    bounds = sorted(set([0, n_groups] + [s for s in splits if 0 < s < n_groups]))
    outs = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        xd = torch.from_numpy(x[:, a * eng.df:b * eng.df].copy()).to(dt).cuda()
        outs.append(eng.run(xd).cpu().numpy().astype(np.int64))
        assert eng.path == expect_path, (eng.path, expect_path, (a, b))
    return np.concatenate(outs, axis=1)


def make(nt, df, fin, fc, fa, fo, coeffs, n_ch, **kw):
    eng = A.PolyDec(nt, df, fin, fc, fa, fo, n_channels=n_ch, **kw)
    eng.set_coeffs(coeffs)
    return eng


def oracle_stream(nt, df, fin, fc, fa, fo, coeffs, x):
    yo = OraclePolyDec(nt, df, ofmt(fin), ofmt(fc), ofmt(fa), ofmt(fo), n_ch=x.shape[0]).run(coeffs, x)
    assert_sat_share(yo, fo, nt, "%d x %d" % (nt, df))
    return yo


def long_case(nt, df, fin, fc, fa, fo, coeffs, n_ch=3, splits_list=((),), seed=0, x=None, expect_path="mfma_long"):
    """one oracle run, one engine stream per call pattern; returns (last engine handle, x, oracle stream)"""
    if x is None:
        x = rand_fmt(np.random.default_rng(seed), fin, (n_ch, stream_groups(nt, df) * df))
    yo = oracle_stream(nt, df, fin, fc, fa, fo, coeffs, x)
    eng = None
    for splits in splits_list:
        eng = make(nt, df, fin, fc, fa, fo, coeffs, n_ch)
        same(run_groups(eng, x, splits, expect_path), yo, "%d x %d, splits %s" % (nt, df, list(splits)))
    return eng, x, yo


# 1. shapes and segment edges.  nb = K-blocks per phase = max(2, ceil((NTAPS-1)/32) + 1); a segment holds 16 of them
@pytest.mark.parametrize("nt,df", [
    (16, 32),      # the first shape past the ring plan; nb 2
    (8, 64),
    (33, 16),      # the last nb = 2
    (34, 16),      # nb 3
    (481, 2),      # nb 16: one full segment
    (482, 3),      # nb 17: a second segment of one block; odd DF
    (1100, 1),     # DF = 1
    (1024, 16),    # 16384 taps, three segments
    (5461, 3),     # 16383 taps
    (64, 256),     # the largest DF
])
def test_shapes_and_segment_edges(nt, df):
    n_ch = 1 if nt * df >= 16383 else 3
    long_case(nt, df, F16, F16, FA, FO, dense(nt * df), n_ch=n_ch, seed=nt * 1000 + df,
              splits_list=([5, 1040, nt + 600],    # (split points in output groups, taken in ascending order) short calls: the history flips buffers
                           []))                    # one call


# 2. accumulator bound: every product at its largest magnitude and of one sign, 16384 of them
@pytest.mark.parametrize("c,xv", [(-32768, -32768), (32639, 32767)])
def test_int32_plane_sums_hold_16384_extreme_products(c, xv):
    nt, df = 1024, 16
    x = np.full((1, stream_groups(nt, df) * df), xv, dtype=np.int64)
    eng, _, _ = long_case(nt, df, F16, F16, FA, FA, np.full(nt * df, c, dtype=np.int64), n_ch=1, x=x)
    y_last = run_groups(eng, x[:, :df])[0, 0]                # the stream goes on: a full window of extreme products
    assert y_last == nt * df * c * xv, (y_last, nt * df * c * xv)


# 3. channel rows: two workgroup rows, the second with one live wave
def test_nine_channels_fill_two_workgroup_rows():
    long_case(16, 32, F16, F16, FA, FO, dense(16 * 32, seed=2), n_ch=9, seed=3, splits_list=([700],))


# 4. time slabs and channel groups
def test_slabs_and_groups_under_a_small_scratch_cap():
    nt, df, n_ch = 16, 32, 17
    c = dense(nt * df, seed=4)
    x = rand_fmt(np.random.default_rng(5), F16, (n_ch, stream_groups(nt, df) * df))
    yo = oracle_stream(nt, df, F16, F16, FA, FO, c, x)
    per_channel = df * (32 + 1024) * 2                       # bytes of the phase rows of one channel at a slab of 1024 outputs (H = 32)
    for splits in ([], [1000, 1100]):
        eng = make(nt, df, F16, F16, FA, FO, c, n_ch)
        assert eng.long_geometry()[1] == n_ch                # default cap: one group
        eng.set_scratch_cap(8 * per_channel)
        assert eng.long_geometry() == (1024, 8, 8 * per_channel), eng.long_geometry()
        same(run_groups(eng, x, splits), yo, "three groups x slabs of 1024, splits %s" % splits)
    same(run_groups(make(nt, df, F16, F16, FA, FO, c, n_ch), x), yo, "default cap")
    ring = make(16, 8, F16, F16, FA, FO, dense(16 * 8, seed=6), 2)
    assert ring.long_geometry() == (0, 0, 0)
    ring.set_scratch_cap(1 << 20)                            # a handle that is not long: accepted, nothing happens
    assert ring.long_geometry() == (0, 0, 0)


# 5. epilogue: containers of 2, 4 and 8 bytes, an accumulator that wraps, an unsigned one (the pairs of test_fir_long_gpu.py at 2049 taps)
@pytest.mark.parametrize("fa,fo", [
    (FA, A.Fmt(16, 10)),
    (FA, A.Fmt(24, 12, True, "RND_CONV", "SAT_SYM")),
    (FA, A.Fmt(48, 20, True, "TRN", "WRAP")),
    (A.Fmt(34, 6), FO),                                       # F = 28: exact products, the sum wraps the 6 integer bits legitimately
    (A.Fmt(48, 20, False), A.Fmt(48, 20, True, "TRN", "WRAP")),
])
def test_epilogue_types_at_129_x_16(fa, fo):
    long_case(129, 16, F16, F16, fa, fo, dense(129 * 16), splits_list=([700],), seed=7)


# 6. samples and coefficients
def test_unsigned_16_bit_samples():
    # the DC term 32768 * sum(c) of a dense set would saturate <16,10>: a 24-bit output keeps every word visible
    long_case(65, 32, A.Fmt(16, 3, False), F16, FA, A.Fmt(24, 12, True, "RND", "SAT"), dense(65 * 32, seed=8), splits_list=([1, 1500],), seed=9)


def test_narrow_samples_and_coefficients():
    fin, fc = A.Fmt(12, 4), A.Fmt(10, 2)
    c = rand_fmt(np.random.default_rng(10), fc, (100 * 30,))
    long_case(100, 30, fin, fc, FA, A.Fmt(24, 12, True, "RND", "SAT"), c, splits_list=([77],), seed=11)


# 7. saturating accumulators
FSAT = A.Fmt(40, 12, True, "TRN", "SAT")


def test_a_saturating_accumulator_that_cannot_saturate_runs_the_long_kernel():
    long_case(256, 16, F16, F16, FSAT, FO, sinc_set(256, 16), splits_list=([300],), seed=12)


def test_a_saturating_accumulator_that_may_saturate_is_refused_above_2048_taps_and_runs_as_before_below():
    nt, df = 256, 16
    eng = A.PolyDec(nt, df, F16, F16, FSAT, FO, n_channels=2)
    with pytest.raises(A.AcdspError) as e:
        eng.set_coeffs(dense(nt * df))
    assert e.value.code == 2, e.value
    x = rand_fmt(np.random.default_rng(13), F16, (2, 300 * df))
    with pytest.raises(A.AcdspError):                        # the handle is left without a set
        run_groups(eng, x)
    # 128 x 16 = 2048 taps: the same kind of set keeps the exact-order kernel
    long_case(128, 16, F16, F16, FSAT, FO, dense(128 * 16), n_ch=2, splits_list=([100],), seed=14, expect_path="generic")


# 8. a coefficient that does not split into two signed bytes
def test_a_coefficient_that_does_not_split_into_two_signed_bytes():
    c = dense(129 * 16)
    c[100] = 32700
    eng = A.PolyDec(129, 16, F16, F16, FA, FO, n_channels=1)
    with pytest.raises(A.AcdspError) as e:
        eng.set_coeffs(c)
    assert e.value.code == 2, e.value
    long_case(64, 16, F16, F16, FA, FO, c[:64 * 16], n_ch=1, seed=15, expect_path="generic")


# 9. cross-path parity: the long kernels and the exact-order kernel of one shape
def test_the_long_path_and_the_exact_order_kernel_agree():
    nt, df, n_ch = 16, 32, 3
    c = dense(nt * df, seed=16)
    _, x, yo = long_case(nt, df, F16, F16, FA, FO, c, n_ch=n_ch, seed=17, splits_list=([900],))
    gen = make(nt, df, F16, F16, FA, FO, c, n_ch, force_generic=True)
    same(run_groups(gen, x, [900], "generic"), yo, "force_generic")


# 10. rows off alignment: an element-aligned slice of a wider buffer with an odd stride
def test_rows_at_any_element_aligned_address_and_stride():
    nt, df, n_ch = 34, 16, 3
    c = dense(nt * df, seed=18)
    x = rand_fmt(np.random.default_rng(19), F16, (n_ch, stream_groups(nt, df) * df))
    yo = oracle_stream(nt, df, F16, F16, FA, FO, c, x)
    eng = make(nt, df, F16, F16, FA, FO, c, n_ch)
    outs, pos = [], 0
    for n in (700 * df, x.shape[1] - 700 * df):
        width = n + 8 + (n % 2 == 0)                         # an odd row stride
        buf = torch.zeros((n_ch, width), dtype=torch.int16, device="cuda")
        xd = buf[:, 3:3 + n]
        xd.copy_(torch.from_numpy(x[:, pos:pos + n].copy()).to(torch.int16))
        assert xd.stride(0) % 2 == 1 and xd.data_ptr() % 4 == 2
        outs.append(eng.run(xd).cpu().numpy().astype(np.int64))
        assert eng.path == "mfma_long", eng.path
        pos += n
    same(np.concatenate(outs, axis=1), yo, "odd stride, rows 6 bytes off")


# 11. stream state at 256 x 16
def test_stream_state_at_256_x_16():
    nt, df, n_ch = 256, 16, 2
    c = dense(nt * df, seed=20)
    rng = np.random.default_rng(21)
    eng = make(nt, df, F16, F16, FA, FO, c, n_ch)
    orc = OraclePolyDec(nt, df, ofmt(F16), ofmt(F16), ofmt(FA), ofmt(FO), n_ch=n_ch)
    stream = []
    for groups in (1, 700, 5000):                            # shorter than the history twice (it flips), then longer (written in place)
        x = rand_fmt(rng, F16, (n_ch, groups * df))
        stream.append(orc.run(c, x))
        same(run_groups(eng, x), stream[-1], "call of %d groups" % groups)
    assert_sat_share(np.concatenate(stream, axis=1), FO, nt, "stream of 1 + 700 + 5000 groups")
    eng.reset()
    x = rand_fmt(rng, F16, (n_ch, 700 * df))
    yo = OraclePolyDec(nt, df, ofmt(F16), ofmt(F16), ofmt(FA), ofmt(FO), n_ch=n_ch).run(c, x)
    assert_sat_share(yo, FO, nt, "after reset()")
    same(run_groups(eng, x), yo, "after reset()")


# 12. node layer
def test_node_layer_shards_a_long_decimator():
    nt, df, n_ch = 256, 16, 6
    c = dense(nt * df, seed=22)
    rng = np.random.default_rng(23)
    node = A.NodePolyDec(nt, df, F16, F16, FA, FO, n_ch, [0, 0])
    node.set_coeffs(c)
    assert node.slices == [(0, 3), (3, 6)]
    orc = OraclePolyDec(nt, df, ofmt(F16), ofmt(F16), ofmt(FA), ofmt(FO), n_ch=n_ch)
    stream = []
    for groups in (1300, 1024):
        x = rand_fmt(rng, F16, (n_ch, groups * df))
        xs = [torch.from_numpy(x[lo:hi].copy()).to(torch.int16).cuda() for lo, hi in node.slices]
        ys = node.run(xs)
        torch.cuda.synchronize()
        stream.append(orc.run(c, x))
        same(np.concatenate([y.cpu().numpy().astype(np.int64) for y in ys]), stream[-1], "node call of %d groups" % groups)
        paths = [PATHS[lib.acdsp_polydec_path(node.shard_handle(s))] for s in range(len(node.slices))]
        assert paths == ["mfma_long"] * 2, paths
    assert_sat_share(np.concatenate(stream, axis=1), FO, nt, "node stream")
    node.close()


# 13. graph capture: no allocation, no synchronisation, no host state beyond the history flip
def test_long_polydec_calls_replayed_from_a_graph_continue_the_stream():
    nt, df, n_ch = 129, 16, 3
    c = dense(nt * df, seed=24)

    def mk():
        return make(nt, df, F16, F16, FA, FO, c, n_ch)

    streams = []                                             # the oracle's outputs, call by call, of every oracle the helper makes

    def oracle():
        o = OraclePolyDec(nt, df, ofmt(F16), ofmt(F16), ofmt(FA), ofmt(FO), n_ch=n_ch)
        streams.append([])

        def run(x, out=streams[-1]):
            out.append(o.run(c, x))
            return out[-1]
        return run

    case = GraphCase(mk, lambda e, xd: e.run(xd), oracle, F16, lambda e: e.path)
    n = 1100 * df                                            # longer than the history (2080 samples): written in place, one call per replay
    rng = np.random.default_rng(25)
    graph_replays_match_oracle(case, [rand_fmt(rng, F16, (n_ch, 300 * df))], chunks_of(26, F16, n_ch, [n]), rand_fmt(rng, F16, (n_ch, 77 * df)), "mfma_long")
    assert streams and all(len(s) > 0 for s in streams)
    for s in streams:                                        # (chunks_of puts full-scale runs into the first rows: the guard matters here)
        assert_sat_share(np.concatenate(s, axis=1), FO, nt, "graph stream")
