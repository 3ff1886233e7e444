"""GPU parity tests, long ac_poly_intr sub-filters (polyintr_long.hip: nt = NTAPS + lag = 65 .. 16384 taps per phase of the exact-accumulation
class on 16-bit types, IF up to 255): the HIP engine against the CPU oracle, bit for bit over the whole stream.

A case streams nt + 2 * 1024 + 77 input samples (nt + 1024 + 77 from 8192 taps on, for the oracle's time): every tap of every phase sees
data, and the stream holds two complete 1024-sample steps and a ragged one.  Dense sets are drawn from [-32768, 32639]; sets used with
symmetric pairs (corr[j] = IF-1-j, every sign set) from [-16000, 16000), so that every pair difference splits into two signed bytes.  Every
case asserts that the oracle's outputs past the first nt * IF sit on a bound of OUT_TYPE in at most 20 % of the positions (measured: at most
0.33 % for these sets).  The path is asserted after every call."""
import numpy as np
import pytest
import torch

import ac_dsp_amd as A
from ac_dsp_amd._lib import lib, PATHS
from oracle import OraclePolyIntr
from helpers import ofmt, rand_fmt, GraphCase, graph_replays_match_oracle
from test_graph_paths_gpu import chunks_of

pytestmark = pytest.mark.gpu

F16 = A.Fmt(16, 2)
FA = A.Fmt(48, 20)                          # F = 28 = F_in + F_coeff: exact products, 19 integer bits of headroom
FO = A.Fmt(16, 10, True, "RND", "SAT")
LAG = {"FOLD_EVEN": 1, "FOLD_ODD": 1, "FOLD_ANTI": 0}


def table_size(n_taps, ifac, ftype):
    j = ifac - 1
    return {"FOLD_EVEN": (n_taps // 2 - 1) + j * n_taps // 2, "FOLD_ODD": (n_taps - 1) // 2 + (n_taps // 2 + 1) * j,
            "FOLD_ANTI": (n_taps - 1) + n_taps * j}[ftype] + 1


def stream_len(nt):
    return nt + (1024 if nt >= 8192 else 2 * 1024) + 77


def ctrl(n_taps, ifac, ftype, pairs, seed=1, fc=F16):
    """(coeffs, sign, corr): a dense table, or one whose pair differences split into two signed bytes"""
    rng = np.random.default_rng(seed)
    csz = table_size(n_taps, ifac, ftype)
    if fc.W < 16:
        c = rand_fmt(rng, fc, (csz,))
    elif pairs:
        c = rng.integers(-16000, 16000, size=csz, dtype=np.int64)
    else:
        c = rng.integers(-32768, 32640, size=csz, dtype=np.int64)
    corr = (ifac - 1 - np.arange(ifac)) if pairs else np.arange(ifac)
    return c, np.ones(ifac, dtype=np.int64), corr


def sat_share(yo, fo, fill):
    """share of the oracle's outputs past the first `fill` that sit on a bound of OUT_TYPE"""
    lo = -(1 << (fo.W - 1)) if fo.S else 0
    hi = (1 << (fo.W - 1)) - 1 if fo.S else (1 << fo.W) - 1
    tail = yo[:, fill:]
    return float(np.mean((tail <= lo + 1) | (tail >= hi))) if tail.size else 0.0


def assert_sat_share(yo_stream, fo, fill, what):
    """the guard of every case: the oracle's whole stream (calls concatenated) is not mostly clamped outputs"""
    share = sat_share(yo_stream, fo, fill)
    print("%s: saturated share past the fill %.4f" % (what, share))
    assert share <= 0.20, (what, share)


def same(y, yo, what=""):
    assert y.shape == yo.shape, (what, y.shape, yo.shape)
    bad = np.argwhere(y != yo)
    assert bad.size == 0, "%s: %d mismatches, first at %s: got %d want %d" % (what, len(bad), bad[0], y[tuple(bad[0])], yo[tuple(bad[0])])


def run_stream(eng, x, splits=(), expect_path="mfma_long"):
    """x: [n_ch][n] raw words -> raw outputs; one call per piece between the split points (in input samples); the path after every call"""
    dt = A.torch_dtype_for(eng.fin)
    n = x.shape[1]
    bounds = sorted(set([0, n] + [s for s in splits if 0 < s < n]))
    outs = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        xd = torch.from_numpy(x[:, a:b].copy()).to(dt).cuda()
        outs.append(eng.run(xd).cpu().numpy().astype(np.int64))
        assert eng.path == expect_path, (eng.path, expect_path, (a, b))
    return np.concatenate(outs, axis=1)


def make(n_taps, ifac, ftype, fin, fc, fa, fo, cs, n_ch, **kw):
    eng = A.PolyIntr(n_taps, len(cs[0]), ifac, ftype, fin, fc, fa, fo, n_channels=n_ch, **kw)
    eng.set_ctrl(*cs)
    return eng


def oracle_of(n_taps, ifac, ftype, fin, fc, fa, fo, cs, n_ch):
    return OraclePolyIntr(n_taps, len(cs[0]), ifac, ftype, ofmt(fin), ofmt(fc), ofmt(fa), ofmt(fo), n_ch=n_ch)


def oracle_stream(n_taps, ifac, ftype, fin, fc, fa, fo, cs, x):
    yo = oracle_of(n_taps, ifac, ftype, fin, fc, fa, fo, cs, x.shape[0]).run(cs[0], cs[1], cs[2], x)
    assert_sat_share(yo, fo, (n_taps + LAG[ftype]) * ifac, "%d x %d %s" % (n_taps, ifac, ftype))
    return yo


def long_case(n_taps, ifac, ftype, fin, fc, fa, fo, cs, n_ch=3, splits_list=((),), seed=0, x=None, expect_path="mfma_long", **kw):
    """one oracle run, one engine stream per call pattern; returns (last engine handle, x, oracle stream)"""
    if x is None:
        x = rand_fmt(np.random.default_rng(seed), fin, (n_ch, stream_len(n_taps + LAG[ftype])))
    yo = oracle_stream(n_taps, ifac, ftype, fin, fc, fa, fo, cs, x)
    eng = None
    for splits in splits_list:
        eng = make(n_taps, ifac, ftype, fin, fc, fa, fo, cs, n_ch, **kw)
        same(run_stream(eng, x, splits, expect_path), yo, "%d x %d %s, splits %s" % (n_taps, ifac, ftype, list(splits)))
    return eng, x, yo


# 1. shapes and segment edges.  nb = K-blocks per phase = max(2, ceil((nt-1)/32) + 1), nt = NTAPS + lag; a segment holds 16 of them
@pytest.mark.parametrize("n_taps,ifac,ftype,pairs", [
    (64, 4, "FOLD_EVEN", True),        # nt 65: the first long shape, nb 3
    (65, 9, "FOLD_ANTI", False),       # an IF fir_up.hip does not compile
    (96, 32, "FOLD_ODD", True),
    (480, 2, "FOLD_EVEN", True),       # nb 16: one full segment
    (482, 3, "FOLD_ANTI", False),      # nb 17: a second segment of one block; odd IF
    (1100, 1, "FOLD_ODD", False),      # IF = 1
    (2048, 8, "FOLD_ANTI", False),
    (8192, 2, "FOLD_EVEN", True),
    (16383, 1, "FOLD_ODD", False),     # nt 16384
    (64, 255, "FOLD_EVEN", False),     # the largest IF, 765 K-blocks
])
def test_shapes_and_segment_edges(n_taps, ifac, ftype, pairs):
    nt = n_taps + LAG[ftype]
    n_ch = 1 if n_taps >= 8192 else 3
    long_case(n_taps, ifac, ftype, F16, F16, FA, FO, ctrl(n_taps, ifac, ftype, pairs, seed=n_taps + ifac), n_ch=n_ch, seed=n_taps * 1000 + ifac,
              splits_list=([1, 5, 1040, nt + 600],   # short calls: a one-sample first call, the history flips buffers
                           []))                      # one call


def test_63_taps_stay_on_the_path_they_had():
    """nt = 64: the boundary from below (fir_up.hip has no plan for 64 taps per phase at IF = 4: the tiled int64 kernel, as before)"""
    long_case(63, 4, "FOLD_EVEN", F16, F16, FA, FO, ctrl(63, 4, "FOLD_EVEN", True, seed=2), seed=3, splits_list=([],), expect_path="lossless64")


# 2. accumulator bound: every product at its largest magnitude and of one sign, 16384 of them
@pytest.mark.parametrize("c,xv", [(-32768, -32768), (32639, 32767)])
def test_int32_plane_sums_hold_16384_extreme_products(c, xv):
    n_taps = 16384
    x = np.full((1, stream_len(n_taps)), xv, dtype=np.int64)
    cs = (np.full(n_taps, c, dtype=np.int64), np.ones(1, dtype=np.int64), np.zeros(1, dtype=np.int64))
    _, _, yo = long_case(n_taps, 1, "FOLD_ANTI", F16, F16, FA, FA, cs, n_ch=1, x=x)
    assert yo[0, -1] == n_taps * c * xv, (yo[0, -1], n_taps * c * xv)       # a full window of extreme products (the engine equals the oracle)


# 3. channel rows: two workgroup rows, the second with one live wave
def test_nine_channels_fill_two_workgroup_rows():
    long_case(64, 4, "FOLD_EVEN", F16, F16, FA, FO, ctrl(64, 4, "FOLD_EVEN", True, seed=4), n_ch=9, seed=5, splits_list=([700],))


# 4. time slabs and channel groups
def test_slabs_and_groups_under_a_small_scratch_cap():
    n_taps, ifac, ft, n_ch = 64, 4, "FOLD_EVEN", 17
    cs = ctrl(n_taps, ifac, ft, True, seed=6)
    x = rand_fmt(np.random.default_rng(7), F16, (n_ch, stream_len(n_taps + 1)))
    yo = oracle_stream(n_taps, ifac, ft, F16, F16, FA, FO, cs, x)
    per_channel = ifac * 1024 * 2                            # bytes of the phase rows of one channel at a slab of 1024 samples
    for splits in ([], [1000, 1100]):
        eng = make(n_taps, ifac, ft, F16, F16, FA, FO, cs, n_ch)
        assert eng.long_geometry()[1] == n_ch                # default cap: one group
        eng.set_scratch_cap(8 * per_channel)
        assert eng.long_geometry() == (1024, 8, 65536), eng.long_geometry()
        same(run_stream(eng, x, splits), yo, "three groups x slabs of 1024, splits %s" % splits)
    same(run_stream(make(n_taps, ifac, ft, F16, F16, FA, FO, cs, n_ch), x), yo, "default cap")
    short = make(16, 4, ft, F16, F16, FA, FO, ctrl(16, 4, ft, True, seed=8), 2)
    assert short.long_geometry() == (0, 0, 0)
    short.set_scratch_cap(1 << 20)                           # a handle that is not long: accepted, nothing happens
    assert short.long_geometry() == (0, 0, 0)


# 5. epilogue: containers of 2, 4 and 8 bytes, a 64-bit accumulator; the pair sets make odd sums under the halving
@pytest.mark.parametrize("fa,fo", [
    (FA, A.Fmt(16, 10)),
    (FA, A.Fmt(24, 12, True, "RND_CONV", "SAT_SYM")),
    (FA, A.Fmt(48, 20)),
    (A.Fmt(64, 32), FO),                                     # 62-bit bound of the control words (acc64_ok)
])
def test_epilogue_types_at_129_x_4(fa, fo):
    long_case(129, 4, "FOLD_EVEN", F16, F16, fa, fo, ctrl(129, 4, "FOLD_EVEN", True, seed=9), splits_list=([700],), seed=10)


# 6. narrow samples and coefficients
def test_narrow_samples_and_coefficients():
    fin, fc = A.Fmt(12, 4), A.Fmt(10, 2)
    long_case(100, 30, "FOLD_ANTI", fin, fc, FA, A.Fmt(24, 12, True, "RND", "SAT"), ctrl(100, 30, "FOLD_ANTI", False, seed=11, fc=fc), splits_list=([77],), seed=12)


# 7. ineligible sets
def _sign0(cs):
    sign = cs[1].copy()
    sign[1] = 0
    return cs[0], sign, cs[2]


def _pair_difference_32700(cs, n_taps, ifac):
    c = cs[0].copy()
    c[0], c[(ifac - 1) * n_taps // 2] = 16350, -16350           # tap 0 of phases 0 and IF-1 (FOLD_EVEN): the folded taps are +/-32700
    return c, cs[1], cs[2]


def test_ineligible_sets_of_up_to_2048_taps_stay_exact_on_the_old_kernel():
    n_taps, ifac, ft = 129, 4, "FOLD_EVEN"
    cs = ctrl(n_taps, ifac, ft, True, seed=13)
    long_case(n_taps, ifac, ft, F16, F16, FA, FO, _sign0(cs), seed=14, splits_list=([700],), expect_path="lossless64")
    long_case(n_taps, ifac, ft, F16, F16, FA, FO, _pair_difference_32700(cs, n_taps, ifac), seed=15, splits_list=([700],), expect_path="lossless64")
    # 34 bits for sums of up to 2^36: the accumulator may wrap, and the pair halving does not commute with a wrap
    long_case(n_taps, ifac, ft, F16, F16, A.Fmt(34, 6), FO, cs, seed=16, splits_list=([700],), expect_path="lossless64")


def test_ineligible_sets_above_2048_taps_are_refused_and_leave_the_handle_as_it_was():
    n_taps, ifac, ft, n_ch = 2100, 4, "FOLD_EVEN", 3
    cs = ctrl(n_taps, ifac, ft, True, seed=17)
    x = rand_fmt(np.random.default_rng(18), F16, (n_ch, stream_len(n_taps + 1)))
    yo = oracle_stream(n_taps, ifac, ft, F16, F16, FA, FO, cs, x)
    eng = make(n_taps, ifac, ft, F16, F16, FA, FO, cs, n_ch)
    cut = n_taps + 700
    y0 = run_stream(eng, x[:, :cut])
    for bad in (_sign0(cs), _pair_difference_32700(cs, n_taps, ifac)):
        with pytest.raises(A.AcdspError) as e:
            eng.set_ctrl(*bad)
        assert e.value.code == 2, e.value
    same(np.concatenate([y0, run_stream(eng, x[:, cut:])], axis=1), yo, "the stream goes on with the good set")
    fresh = A.PolyIntr(n_taps, len(cs[0]), ifac, ft, F16, F16, FA, FO, n_channels=1)
    with pytest.raises(A.AcdspError) as e:
        fresh.set_ctrl(*_sign0(cs))
    assert e.value.code == 2, e.value


# 8. control reload mid-stream: the group behind each reload carries the sums of the old set, combined with the new sign / corr; the
#    second set leaves the long path (a phase with sign = 0) and the third returns to it
def test_control_reload_mid_stream_across_the_paths():
    n_taps, ifac, ft, n_ch = 129, 4, "FOLD_EVEN", 3
    x = rand_fmt(np.random.default_rng(19), F16, (n_ch, stream_len(n_taps + 1)))
    sets = [ctrl(n_taps, ifac, ft, True, seed=20),
            (ctrl(n_taps, ifac, ft, False, seed=21)[0] // 2, np.array([0, 1, 1, 1]), np.arange(ifac)),
            (ctrl(n_taps, ifac, ft, True, seed=22)[0], np.ones(ifac, dtype=np.int64), np.array([1, 0, 3, 2]))]
    paths = ["mfma_long", "lossless64", "mfma_long"]
    eng = A.PolyIntr(n_taps, len(sets[0][0]), ifac, ft, F16, F16, FA, FO, n_channels=n_ch)
    orc = oracle_of(n_taps, ifac, ft, F16, F16, FA, FO, sets[0], n_ch)
    ys, yos = [], []
    for k, (a, b) in enumerate([(0, 900), (900, 901), (901, x.shape[1])]):
        eng.set_ctrl(*sets[k])
        ys.append(run_stream(eng, x[:, a:b], expect_path=paths[k]))
        yos.append(orc.run(sets[k][0], sets[k][1], sets[k][2], x[:, a:b]))
    yo = np.concatenate(yos, axis=1)
    assert_sat_share(yo, FO, (n_taps + 1) * ifac, "three sets")
    same(np.concatenate(ys, axis=1), yo, "three calls, three sets")
    # ... and two long sets back to back: the first group of the second call still carries the first set's sums
    eng = A.PolyIntr(n_taps, len(sets[0][0]), ifac, ft, F16, F16, FA, FO, n_channels=n_ch)
    orc = oracle_of(n_taps, ifac, ft, F16, F16, FA, FO, sets[0], n_ch)
    ys, yos = [], []
    for k, (a, b) in zip((0, 2, 0), [(0, 900), (900, 901), (901, 2000)]):
        eng.set_ctrl(*sets[k])
        ys.append(run_stream(eng, x[:, a:b]))
        yos.append(orc.run(sets[k][0], sets[k][1], sets[k][2], x[:, a:b]))
    same(np.concatenate(ys, axis=1), np.concatenate(yos, axis=1), "long sets back to back")


# 9. cross-path parity: the long kernels and the exact-order kernel of one shape
def test_the_long_path_and_the_exact_order_kernel_agree():
    n_taps, ifac, ft = 64, 4, "FOLD_EVEN"
    cs = ctrl(n_taps, ifac, ft, True, seed=23)
    _, x, yo = long_case(n_taps, ifac, ft, F16, F16, FA, FO, cs, seed=24, splits_list=([900],))
    gen = make(n_taps, ifac, ft, F16, F16, FA, FO, cs, 3, force_generic=True)
    same(run_stream(gen, x, [900], "generic"), yo, "force_generic")


# 10. rows off alignment: element-aligned slices of wider buffers with odd strides, input and output
@pytest.mark.parametrize("ifac", [4, 3])
def test_rows_at_any_element_aligned_address_and_stride(ifac):
    n_taps, ft, n_ch = 98, "FOLD_EVEN", 3
    cs = ctrl(n_taps, ifac, ft, True, seed=25)
    x = rand_fmt(np.random.default_rng(26), F16, (n_ch, stream_len(n_taps + 1)))
    yo = oracle_stream(n_taps, ifac, ft, F16, F16, FA, FO, cs, x)
    eng = make(n_taps, ifac, ft, F16, F16, FA, FO, cs, n_ch)
    outs, pos = [], 0
    for n in (701, x.shape[1] - 701):
        width = n + 8 + (n % 2 == 0)                         # an odd row stride
        buf = torch.zeros((n_ch, width), dtype=torch.int16, device="cuda")
        xd = buf[:, 3:3 + n]
        xd.copy_(torch.from_numpy(x[:, pos:pos + n].copy()).to(torch.int16))
        assert xd.stride(0) % 2 == 1 and xd.data_ptr() % 4 == 2
        no = eng.out_count(n)
        owidth = no + 8 + (no % 2 == 0)
        obuf = torch.full((n_ch, owidth), 12345, dtype=torch.int16, device="cuda")
        od = obuf[:, 3:3 + no]
        assert od.stride(0) % 2 == 1 and od.data_ptr() % 4 == 2
        outs.append(eng.run(xd, out=od).cpu().numpy().astype(np.int64))
        assert eng.path == "mfma_long", eng.path
        guard = obuf.cpu().numpy()
        assert (guard[:, :3] == 12345).all() and (guard[:, 3 + no:] == 12345).all(), "a store outside the caller's rows"
        pos += n
    same(np.concatenate(outs, axis=1), yo, "odd strides, rows 6 bytes off")


# 11. stream state at 256 x 8
def test_stream_state_at_256_x_8():
    n_taps, ifac, ft, n_ch = 256, 8, "FOLD_ODD", 2
    cs = ctrl(n_taps, ifac, ft, False, seed=27)
    rng = np.random.default_rng(28)
    eng = make(n_taps, ifac, ft, F16, F16, FA, FO, cs, n_ch)
    orc = oracle_of(n_taps, ifac, ft, F16, F16, FA, FO, cs, n_ch)
    stream = []
    for n in (1, 700, 5000):                                 # a first call that emits nothing; shorter than the history; longer
        x = rand_fmt(rng, F16, (n_ch, n))
        stream.append(orc.run(cs[0], cs[1], cs[2], x))
        same(run_stream(eng, x), stream[-1], "call of %d samples" % n)
    assert_sat_share(np.concatenate(stream, axis=1), FO, (n_taps + 1) * ifac, "stream of 1 + 700 + 5000 samples")
    eng.reset()
    x = rand_fmt(rng, F16, (n_ch, 700))
    yo = oracle_of(n_taps, ifac, ft, F16, F16, FA, FO, cs, n_ch).run(cs[0], cs[1], cs[2], x)
    assert_sat_share(yo, FO, (n_taps + 1) * ifac, "after reset()")
    same(run_stream(eng, x), yo, "after reset()")


# 12. node layer
def test_node_layer_shards_a_long_interpolator():
    n_taps, ifac, ft, n_ch = 256, 8, "FOLD_EVEN", 6
    cs = ctrl(n_taps, ifac, ft, True, seed=29)
    rng = np.random.default_rng(30)
    node = A.NodePolyIntr(n_taps, len(cs[0]), ifac, ft, F16, F16, FA, FO, n_ch, [0, 0])
    node.set_ctrl(*cs)
    assert node.slices == [(0, 3), (3, 6)]
    orc = oracle_of(n_taps, ifac, ft, F16, F16, FA, FO, cs, n_ch)
    stream = []
    for n in (1300, 1024):
        x = rand_fmt(rng, F16, (n_ch, n))
        xs = [torch.from_numpy(x[lo:hi].copy()).to(torch.int16).cuda() for lo, hi in node.slices]
        ys = node.run(xs)
        torch.cuda.synchronize()
        stream.append(orc.run(cs[0], cs[1], cs[2], x))
        same(np.concatenate([y.cpu().numpy().astype(np.int64) for y in ys]), stream[-1], "node call of %d samples" % n)
        paths = [PATHS[lib.acdsp_polyintr_path(node.shard_handle(s))] for s in range(len(node.slices))]
        assert paths == ["mfma_long"] * 2, paths
    assert_sat_share(np.concatenate(stream, axis=1), FO, (n_taps + 1) * ifac, "node stream")
    node.close()


# 13. graph capture behind an eager first call: no allocation, no synchronisation; the state flips every call -> pairs
def test_long_polyintr_calls_replayed_from_a_graph_continue_the_stream():
    n_taps, ifac, ft, n_ch = 129, 4, "FOLD_EVEN", 3
    cs = ctrl(n_taps, ifac, ft, True, seed=31)

    def mk():
        return make(n_taps, ifac, ft, F16, F16, FA, FO, cs, n_ch)

    streams = []                                             # the oracle's outputs, call by call, of every oracle the helper makes

    def oracle():
        o = oracle_of(n_taps, ifac, ft, F16, F16, FA, FO, cs, n_ch)
        streams.append([])

        def run(x, out=streams[-1]):
            out.append(o.run(cs[0], cs[1], cs[2], x))
            return out[-1]
        return run

    case = GraphCase(mk, lambda e, xd: e.run(xd), oracle, F16, lambda e: e.path)
    rng = np.random.default_rng(32)
    graph_replays_match_oracle(case, [rand_fmt(rng, F16, (n_ch, 300))], chunks_of(33, F16, n_ch, [1100, 1100]), rand_fmt(rng, F16, (n_ch, 77)), "mfma_long")
    assert streams and all(len(s) > 0 for s in streams)
    for s in streams:                                        # (chunks_of puts full-scale runs into the first rows: the guard matters here)
        assert_sat_share(np.concatenate(s, axis=1), FO, (n_taps + 1) * ifac, "graph stream")
