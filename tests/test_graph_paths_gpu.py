"""GPU tests: run() calls of every operator family and kernel path captured into a HIP graph, replayed, and compared bit for bit with the CPU
oracle's continuation of the same stream (tests/test_graph_gpu.py compares four handles with an eager run of the same library).

Section 1 (…_replays_match_the_oracle): each case brings two handles to a pre-capture state with eager calls, captures nk calls of one of them
on a side stream, replays the graph three times on changed input contents, and runs one more eager call behind the last replay.  Every replay,
the eager twin and the trailing call must equal the oracle; the path (or FIR kernel class) of every captured call is pinned.  The type sets
are those of tests/pathmap_grid.py / tests/pathmap_ops.py, whose golden tables say which kernel each of them reaches.  Calls of at least `hl`
samples update the history in place, so an odd number of them qualifies; shorter calls flip a double buffer and are captured in pairs, and so
are the calls of handles whose state always flips (reg_trans of a TRANSPOSED filter with loadable coefficients outside the exact-sum class,
ac_poly_intr).

Section 2 (…_refused_under_capture): what a replay cannot repeat is refused with a message that names the graph capture, before the call
touches the stream or the handle: the capture still ends cleanly and replays the legal call in front of the refused one correctly.

The node-level handles (acdsp_node_*) launch on their own streams and are outside these tests."""
import numpy as np
import pytest
import torch

import ac_dsp_amd as A
from oracle import OracleFir, OracleFirW, OracleCic, OraclePolyDec, OraclePolyIntr, OracleIntgDump, OracleMvAvg
from helpers import ofmt, rand_fmt, dev_rows, host_words, GraphCase, graph_replays_match_oracle, refused_under_capture
import pathmap_grid as PG
import pathmap_ops as PO

pytestmark = pytest.mark.gpu

F = A.Fmt


def chunks_of(seed, fmt, rows, lengths):
    """captured(r): replay r's chunks, different contents every replay; full-scale runs in the first rows"""
    def captured(r):
        rng = np.random.default_rng(1000 * seed + r)
        out = [rand_fmt(rng, fmt, (rows, n)) for n in lengths]
        hi = (1 << (fmt.W - 1)) - 1 if fmt.S else (1 << fmt.W) - 1
        out[0][0, : lengths[0] // 2] = hi
        if rows > 1 and fmt.S:
            out[-1][1, lengths[-1] // 3:] = -hi - 1
        return out
    return captured


# ---------------------------------------------------------------------------------------------
# FIR: one case per path / kernel class (keys of tests/golden/path_map.json)
# ---------------------------------------------------------------------------------------------
FIR_CASES = {
    # name: (types, OUT, taps, kind, ftype, coefficient set, per channel, kernel class, long calls)
    "mfma_gen_wide_samples": ("i32_c16", "o16_rnd_sat", 63, "load", "SHIFT_REG", "sinc", False, "mfma_gen", 3),
    "mfma_lossy_class_b": ("i16_lossy_rnd_s4", "o16_rnd_sat", 63, "load", "SHIFT_REG", "sinc", False, "mfma_lossy", 3),
    "lossy16_class_b_valu": ("i16_lossy_rnd_s4", "o16_rnd_sat", 255, "load", "SHIFT_REG", "sinc", False, "lossy16", 3),
    "satacc16_class_c": ("i16_sat_acc", "o16_rnd_sat", 63, "load", "SHIFT_REG", "dense", False, "satacc16", 3),
    "lossless64": ("ddc_stage", "o16_rnd_sat", 63, "load", "SHIFT_REG", "sinc", True, "lossless64", 3),
    "generic": ("i16_conv_acc", "o16_rnd_sat", 63, "load", "SHIFT_REG", "sinc", False, "generic", 3),
    "wide_acc": ("wide_acc", "o16_rnd_sat", 63, "load", "SHIFT_REG", "sinc", False, "wide", 3),
    "unsigned16_in_flip": ("u16", "o16_rnd_sat", 63, "load", "SHIFT_REG", "sinc", False, "mfma_i8", 3),
    "out_4_bytes": ("i16_exact", "o24_rnd_sat", 63, "load", "SHIFT_REG", "sinc", False, "mfma_i8", 3),
    "out_8_bytes": ("i16_exact", "o_acc", 63, "load", "SHIFT_REG", "sinc", False, "mfma_i8", 3),
    "out_16_conv_satsym": ("i16_exact", "o16_conv_satsym", 63, "load", "SHIFT_REG", "sinc", False, "mfma_i8", 3),
    "transposed_load_rt_hybrid": ("i16_exact", "o16_rnd_sat", 63, "load", "TRANSPOSED", "sinc", False, "mfma_i8", 3),
    "transposed_const": ("i16_exact", "o16_rnd_sat", 63, "const", "TRANSPOSED", "sinc", False, "mfma_i8", 3),
    # reg_trans outside the exact-sum class (use_rt): the state flips on every call, long or short -> pairs
    "transposed_load_reg_trans": ("i16_lossy_rnd_s4", "o16_rnd_sat", 63, "load", "TRANSPOSED", "sinc", False, "generic", 2),
}


def fir_case(name, n_ch):
    tname, oname, nt, kind, ftype, sname, per_ch, kclass, nk_long = FIR_CASES[name]
    key = "%s|%s|%d|%s|%s|%s|%d" % (tname, oname, nt, kind, ftype, sname, int(per_ch))
    assert PG_MAP[key].split("/")[0] == kclass, (key, PG_MAP[key])     # the case is the golden table's, not an invention
    fin, fc, fa = PG.TYPES[tname]
    fo = PG.OUTS[oname](fa)
    c = PG.coeffs_of(sname, nt, fc)
    lim = (1 << (fc.W - 1)) - 1
    cc = np.stack([np.clip(c + 3 * i, -lim, lim) for i in range(n_ch)]) if per_ch else c      # (per channel: a set of its own for each)
    wide = fa.W > 64 or fo.W > 64

    def make():
        e = A.Fir(nt, ftype, fin, fc, fa, fo, n_channels=n_ch, kind=kind, coeffs_per_channel=per_ch)
        e.set_coeffs(cc)
        return e

    def oracle():
        o = (OracleFirW if wide else OracleFir)(nt, ftype, ofmt(fin), ofmt(fc), ofmt(fa), ofmt(fo), n_ch=n_ch)
        return lambda x: np.asarray(o.run(cc, x)).astype(np.int64)

    case = GraphCase(make, lambda e, xd: e.run(xd), oracle, fin, lambda e: e.kernel)
    case.fir = (nt, ftype, fin, fc, fa, fo, cc)
    return case, kclass, nt, nk_long


def _load_map(name):
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)) as f:
        return json.load(f)


PG_MAP = _load_map("path_map.json")
PO_MAP = _load_map("path_map_ops.json")


@pytest.mark.parametrize("short", [False, True], ids=["long_calls", "short_pairs"])
@pytest.mark.parametrize("name", list(FIR_CASES))
def test_fir_replays_match_the_oracle(name, short):
    n_ch = 3
    case, kclass, nt, nk_long = fir_case(name, n_ch)
    hl = (nt - 1 + 31) // 32 * 32
    if short:
        lengths = [hl - 16, hl - 16]          # shorter than the history: the double buffer flips, twice
    else:
        lengths = [8192] * nk_long            # whole 4096-sample chunks (the ring kernels of class B) and in-place history updates
    assert all((n < hl) == short for n in lengths)
    seed = list(FIR_CASES).index(name) * 2 + int(short)
    rng = np.random.default_rng(seed)
    # one eager call of more than n_taps - 1 samples in front: the rt_hybrid handle is past its coefficient load, every handle has a history
    pre = [rand_fmt(rng, case.fmt, (n_ch, 2 * hl + 48))]
    post = rand_fmt(rng, case.fmt, (n_ch, 3 * hl + 16))
    graph_replays_match_oracle(case, pre, chunks_of(seed, case.fmt, n_ch, lengths), post, kclass)
    if name == "unsigned16_in_flip":
        assert case.make().mfma_epilogue()[2], "the unsigned samples did not take the sign-flip form of the int8 kernel"


# ---------------------------------------------------------------------------------------------
# CIC decimator
# ---------------------------------------------------------------------------------------------
def cic_case(interp, fin, R, M, N, n_ch, force_generic=False):
    it = A.Cic(bool(interp), R, M, N, fin, fin).int_type
    fo = F(it.W, it.I)

    def oracle():
        o = OracleCic(int(interp), R, M, N, ofmt(fin), ofmt(fo), n_ch=n_ch)
        return lambda x: o.run(x)

    return GraphCase(lambda: A.Cic(bool(interp), R, M, N, fin, fo, n_channels=n_ch, force_generic=force_generic), lambda e, xd: e.run(xd), oracle,
                     fin, lambda e: e.path)


CIC_DEC = {
    # name: (pathmap_ops sample type, R, M, N, force_generic, path of a long call, samples of a long call)
    "two_stage_R64_N3_s16": ("s16", 64, 1, 3, False, "two_stage", 64 * 768),
    "two_stage_R32_N4_s32": ("s32", 32, 2, 4, False, "two_stage", 32 * 1536),
    "recurrence_R37_s16": ("s16", 37, 1, 3, False, "recurrence", 37 * 16 * 64),
    "one_stage_R8_s16": ("s16", 8, 1, 3, False, "mfma_gen", 8192),
    "force_generic_R64_s16": ("s16", 64, 1, 3, True, "recurrence", 64 * 768),
}


@pytest.mark.parametrize("state", ["phase0", "ragged"])
@pytest.mark.parametrize("name", list(CIC_DEC))
def test_cic_decimator_replays_match_the_oracle(name, state):
    """phase0: the handle is primed by one eager call and reset, as a deployment that captures at start-up does.  ragged: one eager call leaves
    the stream at t_total % R = R - 5, so that every captured call starts 5 samples in front of its first output -- window phase first % 16 = 5,
    which no call before the capture has used: the eager call in front of a capture uploads the plan of the phase it leaves behind."""
    iname, R, M, N, fg, path, n_long = CIC_DEC[name]
    if not fg:
        assert PO_MAP["cic|dec|%s|R%d|M%d|N%d|int_type" % (iname, R, M, N)] == path
    fin, n_ch = PO.CIC_IN[iname], 3
    case = cic_case(0, fin, R, M, N, n_ch, fg)
    seed = 100 + list(CIC_DEC).index(name) * 2 + (state == "ragged")
    rng = np.random.default_rng(seed)
    n_pre = n_long if state == "phase0" else n_long + R - 5
    assert state == "phase0" or ((R - n_pre % R) % R) % 16 == 5
    graph_replays_match_oracle(case, [rand_fmt(rng, fin, (n_ch, n_pre))], chunks_of(seed, fin, n_ch, [n_long] * 3), rand_fmt(rng, fin, (n_ch, n_long + 7)),
                               path, reset_after_pre=(state == "phase0"))


@pytest.mark.parametrize("state", ["phase0", "ragged"])
def test_two_stage_decimator_short_calls_in_pairs(state):
    """calls shorter than the two-stage handle's history (4 - 8 K samples): the history flips per call; such calls hold no complete two-stage
    chunk and run the recurrence kernel, from the same long history"""
    fin, R, M, N, n_ch = PO.CIC_IN["s16"], 64, 1, 3, 3
    case = cic_case(0, fin, R, M, N, n_ch)
    rng = np.random.default_rng(77)
    n_pre = 64 * 768 + (0 if state == "phase0" else R - 5)
    eng = case.make()
    eng.run(dev_rows(rand_fmt(rng, fin, (n_ch, 64 * 768)), fin))
    assert eng.path == "two_stage"
    short = 64 * 32
    eng.run(dev_rows(rand_fmt(rng, fin, (n_ch, short)), fin))
    short_path = eng.path            # (pinned below for the captured handle: whatever kernel serves a short eager call serves the captured one)
    assert short_path in ("recurrence", "two_stage")
    del eng
    graph_replays_match_oracle(case, [rand_fmt(rng, fin, (n_ch, n_pre))], chunks_of(78, fin, n_ch, [short, short]), rand_fmt(rng, fin, (n_ch, 64 * 768 + 3)),
                               short_path, n_replays=4)


# ---------------------------------------------------------------------------------------------
# CIC interpolator, PolyDec, PolyIntr, Ddc
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,path", [(8, "mfma_gen"), (10, "fir_identity")])
def test_cic_interpolator_replays_match_the_oracle(R, path):
    """behind its first eager call (which drops the start-up outputs).  R = 8: the matrix-core kernel with the head and tail launches of the
    polyphase kernel in the graph; R = 10: the polyphase VALU kernel alone"""
    assert PO_MAP["cic|intr|s16|R%d|M1|N3|int_type" % R] == path
    fin, n_ch = PO.CIC_IN["s16"], 3
    case = cic_case(1, fin, R, 1, 3, n_ch)
    rng = np.random.default_rng(R)
    graph_replays_match_oracle(case, [rand_fmt(rng, fin, (n_ch, 4096))], chunks_of(200 + R, fin, n_ch, [4096] * 3), rand_fmt(rng, fin, (n_ch, 2048 + 5)), path)


@pytest.mark.parametrize("df", [2, 5, 16])
def test_polydec_replays_match_the_oracle(df):
    from bench import windowed_sinc_raw
    fin, fc, fa = PO.PD_TYPES["i16"]
    fo, tp, n_ch = PO.PD_OUT["o16"], 8, 3
    hh = np.concatenate([windowed_sinc_raw(tp * df - 1, 0.4 / df, fc.W - fc.I), [0]])
    c = np.array([hh[d + t * df] for d in range(df) for t in range(tp)], dtype=np.int64)

    def make():
        e = A.PolyDec(tp, df, fin, fc, fa, fo, n_channels=n_ch)
        e.set_coeffs(c)
        return e

    def oracle():
        o = OraclePolyDec(tp, df, ofmt(fin), ofmt(fc), ofmt(fa), ofmt(fo), n_ch=n_ch)
        return lambda x: o.run(c, x)

    case = GraphCase(make, lambda e, xd: e.run(xd), oracle, fin, lambda e: e.path)
    n = 16 * df * 64
    rng = np.random.default_rng(df)
    graph_replays_match_oracle(case, [rand_fmt(rng, fin, (n_ch, n))], chunks_of(300 + df, fin, n_ch, [n] * 3), rand_fmt(rng, fin, (n_ch, 16 * df * 3)), "mfma_gen")


def test_polyintr_valu_path_replays_match_the_oracle():
    """calls too short for a matrix-core step (fewer than 32 slots of 16 inputs): the tiled int64 VALU kernel; the state flips every call -> pairs"""
    ifac, n_taps, n_ch = 4, 16, 3
    fin, fc, fa, fo = F(16, 2), F(16, 2), F(40, 12), F(16, 2, True, "RND", "SAT")     # (the types of tests/test_graph_gpu.py's mfma_gen cases)
    csz = (n_taps // 2 - 1) + (ifac - 1) * n_taps // 2 + 1
    rng = np.random.default_rng(41)
    c = rng.integers(-3000, 3000, size=csz, dtype=np.int64)
    sign, corr = np.ones(ifac, dtype=np.int64), np.arange(ifac)

    def make():
        e = A.PolyIntr(n_taps, csz, ifac, "FOLD_EVEN", fin, fc, fa, fo, n_channels=n_ch)
        e.set_ctrl(c, sign, corr)
        return e

    def oracle():
        o = OraclePolyIntr(n_taps, csz, ifac, "FOLD_EVEN", ofmt(fin), ofmt(fc), ofmt(fa), ofmt(fo), n_ch=n_ch)
        return lambda x: o.run(c, sign, corr, x)

    case = GraphCase(make, lambda e, xd: e.run(xd), oracle, fin, lambda e: e.path)
    graph_replays_match_oracle(case, [rand_fmt(rng, fin, (n_ch, 256))], chunks_of(42, fin, n_ch, [256, 256]), rand_fmt(rng, fin, (n_ch, 100)), "lossless64", n_replays=4)


def ddc_two_kernels(n_ch):
    from test_ddc_gpu import windowed_sinc
    cin, fc, fa, fo = F(32, 16), F(16, 1), F(64, 31), F(32, 16, True, "RND", "SAT")     # tests/test_ddc_gpu.py: int32 containers -> not the fused class
    c = windowed_sinc(63, 0.2, fc)

    def make():
        d = A.Ddc(8, 1, 5, cin, 63, "SHIFT_REG", fc, fa, fo, n_channels=n_ch)
        d.set_coeffs(c)
        assert d.path == "two_kernels"
        return d

    def oracle():
        mid = make().int_type
        a = OracleCic(False, 8, 1, 5, ofmt(cin), ofmt(mid), n_ch=n_ch)
        b = OracleFir(63, "SHIFT_REG", ofmt(mid), ofmt(fc), ofmt(fa), ofmt(fo), n_ch=n_ch)
        return lambda x: b.run(c, a.run(x))

    return GraphCase(make, lambda e, xd: e.run(xd), oracle, cin, lambda e: e.path)


def test_ddc_two_kernels_replays_match_the_oracle():
    """the intermediate buffer is sized by the eager call of the same length in front of the capture"""
    n_ch, n = 3, 8 * 2048
    case = ddc_two_kernels(n_ch)
    rng = np.random.default_rng(51)
    graph_replays_match_oracle(case, [rand_fmt(rng, case.fmt, (n_ch, n))], chunks_of(52, case.fmt, n_ch, [n] * 3), rand_fmt(rng, case.fmt, (n_ch, 8 * 300 + 3)),
                               "two_kernels")


def fused_ddc(n_ch):
    cin, fc, fa, fo = F(16, 1), F(16, 1), F(60, 30), F(24, 9, True, "RND", "SAT")       # tests/test_graph_gpu.py
    c = np.random.default_rng(9).integers(-3000, 3000, size=127, dtype=np.int64)

    def make():
        d = A.Ddc(16, 1, 5, cin, 127, "SHIFT_REG", fc, fa, fo, n_channels=n_ch)
        d.set_coeffs(c)
        assert d.path == "fused"
        return d

    def oracle():
        mid = make().int_type
        a = OracleCic(False, 16, 1, 5, ofmt(cin), ofmt(mid), n_ch=n_ch)
        b = OracleFir(127, "SHIFT_REG", ofmt(mid), ofmt(fc), ofmt(fa), ofmt(fo), n_ch=n_ch)
        return lambda x: b.run(c, a.run(x))

    return GraphCase(make, lambda e, xd: e.run(xd), oracle, cin, lambda e: e.path)


@pytest.mark.parametrize("state", ["phase0", "ragged"])
def test_fused_ddc_replays_match_the_oracle(state):
    """the fused cascade against the oracle cascade (tests/test_graph_gpu.py compares it with an eager run), also from a stream left mid-period:
    16 * k + 11 inputs in front leave t_total % 16 = 11, window phase 5 (rows stay 16-byte aligned: each call has its own buffer)"""
    n_ch, n = 3, 16 * 256 * 4
    case = fused_ddc(n_ch)
    rng = np.random.default_rng(61)
    n_pre = n + (0 if state == "phase0" else 11)
    graph_replays_match_oracle(case, [rand_fmt(rng, case.fmt, (n_ch, n_pre))], chunks_of(62, case.fmt, n_ch, [n] * 3), rand_fmt(rng, case.fmt, (n_ch, 16 * 300 + 9)),
                               "fused", reset_after_pre=(state == "phase0"))


# ---------------------------------------------------------------------------------------------
# IntgDump, MvAvg
# ---------------------------------------------------------------------------------------------
def intgdump_case(tname, chn, ns, n_obj, n_sample):
    fin, fa, fo = PO.ID_TYPES[tname]

    def oracle():
        o = OracleIntgDump(ns, chn, ofmt(fin), ofmt(fa), ofmt(fo), n_obj=n_obj)
        return lambda x: o.run(x, n_sample)

    return GraphCase(lambda: A.IntgDump(ns, chn, fin, fa, fo, n_objects=n_obj), lambda e, xd: e.run(xd, n_sample), oracle, fin, lambda e: e.path)


@pytest.mark.parametrize("chn,ns,path", [(3, 8, "tile"), (4, 64, "stream"), (3, 64, "mfma")])
def test_intgdump_replays_match_the_oracle(chn, ns, path):
    """every block dumps and the table is that of the eager call in front, which ran on the capture stream (the table is keyed by stream).
    LDS-tiled, streaming and matrix-core kernel (CHN = 3 does not divide a 16-byte load)"""
    assert PO_MAP["intgdump|i16|CHN%d|NS%d" % (chn, ns)] == path
    n_obj = 3
    blocks = max(2, (1 << 14) // (ns * chn))
    n_sample = np.full(blocks, ns, dtype=np.int64)
    case = intgdump_case("i16", chn, ns, n_obj, n_sample)
    n = blocks * ns * chn
    rng = np.random.default_rng(chn * 100 + ns)
    graph_replays_match_oracle(case, [rand_fmt(rng, case.fmt, (n_obj, n))], chunks_of(400 + chn + ns, case.fmt, n_obj, [n] * 3), rand_fmt(rng, case.fmt, (n_obj, n)), path)


MVAVG = {
    # pathmap_ops key -> path; the third: an order-dependent accumulator (tests/test_mvavg_gpu.py) on the exact-order kernel
    "stream": ("i12", 17, "MIRROR", PO.MV_TYPES["i12"] + (F(16, 8, True, "RND", "SAT"),)),
    "stream_mfma": ("i16_sat", 17, "MIRROR", PO.MV_TYPES["i16_sat"] + (F(16, 8, True, "RND", "SAT"),)),
    "exact_order": (None, 7, "MIRROR", (F(24, 12), F(12, 2), F(16, 6, True, "RND_CONV", "SAT"), F(14, 5, True, "RND_CONV", "SAT"))),
}


@pytest.mark.parametrize("path", list(MVAVG))
def test_mvavg_replays_match_the_oracle(path):
    """stateless: one captured call, replayed on changed input contents"""
    tname, taps, mode, (fin, fc, fa, fo) = MVAVG[path]
    if tname:
        assert PO_MAP["mvavg|%s|T%d|%s|ns1024|o16" % (tname, taps, mode)] == path
    n_obj, ns = 3, 1024
    w = np.hanning(taps + 2)[1:-1]
    c = np.round(w / w.sum() * 2.0 ** (fc.W - fc.I)).astype(np.int64)

    def make():
        e = A.MvAvg(4096, taps, mode, fin, fc, fa, fo, n_objects=n_obj)
        e.set_coeffs(c)
        return e

    def oracle():
        o = OracleMvAvg(taps, mode, ofmt(fin), ofmt(fc), ofmt(fa), ofmt(fo), n_obj=n_obj)
        return lambda x: o.run(c, x, ns)

    case = GraphCase(make, lambda e, xd: e.run(xd, ns), oracle, fin, lambda e: e.path)
    rng = np.random.default_rng(taps)
    graph_replays_match_oracle(case, [], chunks_of(500 + taps, fin, n_obj, [8 * ns]), rand_fmt(rng, fin, (n_obj, 3 * ns)), path)


# ---------------------------------------------------------------------------------------------
# Section 2: refused under capture, and the capture survives
# ---------------------------------------------------------------------------------------------
def _replay_and_check(g, y, want):
    y.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    got = host_words(y)
    assert got.shape == want.shape and np.array_equal(got, want), "the legal call in front of the refused one replays wrongly"


def test_rt_hybrid_fir_behind_a_coefficient_load_is_refused_under_capture():
    """a coefficient change mid-stream: the next n_taps - 1 outputs still carry partial sums of the old set (reg_trans), host-side state"""
    n_ch = 3
    case, kclass, nt, _ = fir_case("transposed_load_rt_hybrid", n_ch)
    nt, ftype, fin, fc, fa, fo, c = case.fir
    c2 = np.clip(c[::-1] + 5, -32767, 32767)
    rng = np.random.default_rng(71)
    ok, bad, orc = case.make(), case.make(), case.oracle()
    orc2 = OracleFir(nt, ftype, ofmt(fin), ofmt(fc), ofmt(fa), ofmt(fo), n_ch=n_ch)
    x0, x1 = rand_fmt(rng, fin, (n_ch, 256)), rand_fmt(rng, fin, (n_ch, 4096))
    orc(x0)
    ok.run(dev_rows(x0, fin))
    assert np.array_equal(host_words(bad.run(dev_rows(x0, fin))), orc2.run(c, x0))
    bad.set_coeffs(c2)
    assert np.array_equal(host_words(bad.run(dev_rows(x0[:, :nt - 2], fin))), orc2.run(c2, x0[:, :nt - 2]))     # one sample short of n_taps - 1
    xd = dev_rows(x1, fin)
    g, y, msg = refused_under_capture(lambda: ok.run(xd), lambda: bad.run(xd))
    assert "TRANSPOSED" in msg and "run 1 more samples" in msg, msg
    _replay_and_check(g, y, orc(x1))
    # the refused handle is untouched: it continues eagerly as if the call had never been made
    assert np.array_equal(host_words(bad.run(xd)), orc2.run(c2, x1))


def test_polyintr_first_call_is_refused_under_capture():
    ifac, n_taps, n_ch = 4, 16, 3
    fin, fc, fa, fo = F(16, 2), F(16, 2), F(40, 12), F(16, 2, True, "RND", "SAT")
    csz = (n_taps // 2 - 1) + (ifac - 1) * n_taps // 2 + 1
    rng = np.random.default_rng(72)
    c = rng.integers(-3000, 3000, size=csz, dtype=np.int64)
    sign, corr = np.ones(ifac, dtype=np.int64), np.arange(ifac)

    def make():
        e = A.PolyIntr(n_taps, csz, ifac, "FOLD_EVEN", fin, fc, fa, fo, n_channels=n_ch)
        e.set_ctrl(c, sign, corr)
        return e

    ok, bad = make(), make()
    orc = OraclePolyIntr(n_taps, csz, ifac, "FOLD_EVEN", ofmt(fin), ofmt(fc), ofmt(fa), ofmt(fo), n_ch=n_ch)
    x0, x1 = rand_fmt(rng, fin, (n_ch, 256)), rand_fmt(rng, fin, (n_ch, 256))
    orc.run(c, sign, corr, x0)
    ok.run(dev_rows(x0, fin))
    xd = dev_rows(x1, fin)
    g, y, msg = refused_under_capture(lambda: ok.run(xd), lambda: bad.run(xd))
    assert "first call" in msg, msg
    _replay_and_check(g, y, orc.run(c, sign, corr, x1))


def test_fused_ddc_ragged_call_is_refused_under_capture():
    """the refused call is one of the SAME handle: it must leave the handle's input count and history index alone"""
    n_ch, n = 3, 16 * 256 * 2
    case = fused_ddc(n_ch)
    rng = np.random.default_rng(73)
    d, orc = case.make(), case.oracle()
    x0, x1, x2 = (rand_fmt(rng, case.fmt, (n_ch, n)) for _ in range(3))
    orc(x0)
    d.run(dev_rows(x0, case.fmt))
    xd, xr = dev_rows(x1, case.fmt), dev_rows(rand_fmt(rng, case.fmt, (n_ch, n + 16)), case.fmt)
    g, y, msg = refused_under_capture(lambda: d.run(xd), lambda: d.run(xr[:, :n + 3]))
    assert "multiple of R" in msg, msg
    _replay_and_check(g, y, orc(x1))
    assert np.array_equal(host_words(d.run(dev_rows(x2, case.fmt))), orc(x2))


@pytest.mark.parametrize("family", ["cic", "ddc"])
def test_window_phase_without_an_uploaded_plan_is_refused_under_capture(family):
    """The fir_gen plan of a window phase is uploaded by an eager call (its own phase, the phase it leaves behind, phase 0); a handle that has
    never run eagerly has none, and the upload would synchronise the capturing stream: refused, with the way out in the message."""
    n_ch = 3
    case = cic_case(0, PO.CIC_IN["s16"], 8, 1, 3, n_ch) if family == "cic" else fused_ddc(n_ch)
    n = 8192
    rng = np.random.default_rng(74)
    ok, fresh, orc = case.make(), case.make(), case.oracle()
    x0, x1 = rand_fmt(rng, case.fmt, (n_ch, n)), rand_fmt(rng, case.fmt, (n_ch, n))
    orc(x0)
    ok.run(dev_rows(x0, case.fmt))
    xd = dev_rows(x1, case.fmt)
    g, y, msg = refused_under_capture(lambda: ok.run(xd), lambda: fresh.run(xd))
    assert "one eager call at that phase unlocks it" in msg, msg
    _replay_and_check(g, y, orc(x1))
    # ... and so it does
    orc2 = case.oracle()
    assert np.array_equal(host_words(fresh.run(xd)), orc2(x1))
    out = fresh.run(xd)
    torch.cuda.synchronize()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=torch.cuda.Stream()):
        fresh.run(xd, out=out)
    orc2(x1)
    _replay_and_check(g2, out, orc2(x1))


def test_two_kernel_ddc_with_a_small_intermediate_buffer_is_refused_under_capture():
    """... and an eager call that grows the buffer afterwards leaves the captured graph's buffer alone: the graph still replays"""
    n_ch, n = 3, 8 * 1024
    case = ddc_two_kernels(n_ch)
    rng = np.random.default_rng(75)
    d, orc = case.make(), case.oracle()
    x0, x1, x2, x3 = rand_fmt(rng, case.fmt, (n_ch, n)), rand_fmt(rng, case.fmt, (n_ch, n)), rand_fmt(rng, case.fmt, (n_ch, 4 * n)), rand_fmt(rng, case.fmt, (n_ch, n))
    orc(x0)
    d.run(dev_rows(x0, case.fmt))
    xd, xl = dev_rows(x1, case.fmt), dev_rows(x2, case.fmt)
    g, y, msg = refused_under_capture(lambda: d.run(xd), lambda: d.run(xl))
    assert "intermediate buffer" in msg, msg
    _replay_and_check(g, y, orc(x1))
    assert np.array_equal(host_words(d.run(xl)), orc(x2))       # eager: the buffer grows; the old one stays with the graph
    xd.copy_(torch.from_numpy(x3).to(xd.dtype))
    _replay_and_check(g, y, orc(x3))


def test_fir_rows_that_need_the_staging_image_are_refused_under_capture():
    n_ch = 3
    case, kclass, nt, _ = fir_case("mfma_gen_wide_samples", n_ch)
    rng = np.random.default_rng(76)
    f, orc = case.make(), case.oracle()
    x0, x1, x2 = (rand_fmt(rng, case.fmt, (n_ch, 4096)) for _ in range(3))
    orc(x0)
    f.run(dev_rows(x0, case.fmt))
    xd = dev_rows(x1, case.fmt)
    odd = torch.zeros((n_ch, 4096 + 67), dtype=xd.dtype, device="cuda")[:, 1:4097]      # rows that start on odd elements
    odd.copy_(torch.from_numpy(x2).to(odd.dtype))
    g, y, msg = refused_under_capture(lambda: f.run(xd), lambda: f.run(odd))
    assert "staging image" in msg, msg
    _replay_and_check(g, y, orc(x1))
    assert np.array_equal(host_words(f.run(odd)), orc(x2))       # eager: served through the staging image, which that call sizes ...
    assert f.kernel == kclass
    out = f.run(xd)
    orc(x1)
    torch.cuda.synchronize()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=torch.cuda.Stream()):       # ... so that the same rows can now be captured
        f.run(odd, out=out)
    _replay_and_check(g2, out, orc(x2))
    big = rand_fmt(rng, case.fmt, (n_ch, 3 * 4096))               # an eager call that grows the image leaves the graph's image alone
    oddb = torch.zeros((n_ch, 3 * 4096 + 67), dtype=xd.dtype, device="cuda")[:, 1:3 * 4096 + 1]
    oddb.copy_(torch.from_numpy(big).to(oddb.dtype))
    assert np.array_equal(host_words(f.run(oddb)), orc(big))
    _replay_and_check(g2, out, orc(x2))


@pytest.mark.parametrize("why", ["new_table", "blocks_that_do_not_dump", "sums_pending"])
def test_intgdump_calls_with_host_side_state_are_refused_under_capture(why):
    chn, ns, n_obj, blocks = 4, 64, 3, 32
    tbl = np.full(blocks, ns, dtype=np.int64)
    case = intgdump_case("i16", chn, ns, n_obj, tbl)
    fin = case.fmt
    n = blocks * ns * chn
    rng = np.random.default_rng(77)
    ok, bad = case.make(), case.make()
    orc = case.oracle()
    x0, x1 = rand_fmt(rng, fin, (n_obj, n)), rand_fmt(rng, fin, (n_obj, n))
    xd = dev_rows(x1, fin)
    side = torch.cuda.Stream()
    other = tbl.copy()
    if why == "new_table":
        other[3] = ns // 2                                   # dumps early: another table, every block still dumps
    elif why == "blocks_that_do_not_dump":
        other[5] = 0                                         # N_TYPE 0: block 5 runs NS rounds and leaves its sums to block 6 -- nothing pending at the end
    else:
        other[-1] = 0                                        # ... the last block: its sums are pending when the call returns
    orc(x0)
    with torch.cuda.stream(side):
        ok.run(dev_rows(x0, fin), tbl)
        bad.run(dev_rows(x0, fin), tbl if why == "new_table" else other)     # (the table of the refused call is on the device, on this stream, unless it is the new one)
    side.synchronize()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    msg = None
    with torch.cuda.graph(g, stream=side):
        y = ok.run(xd, tbl)
        try:
            bad.run(xd, other)
        except RuntimeError as e:
            msg = str(e)
    torch.cuda.synchronize()
    assert msg is not None and "graph capture" in msg, msg
    assert {"new_table": "table differs", "blocks_that_do_not_dump": "do not dump", "sums_pending": "pending"}[why] in msg, msg
    _replay_and_check(g, y, orc(x1))
