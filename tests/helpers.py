"""Shared test helpers: golden-vector loading, stimulus, oracle/engine pairing."""
import math
import os
from fractions import Fraction

import numpy as np

from oracle import Fmt as OFmt, from_double

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TXT = os.path.join(GOLD, "ref_txt")


def read_fracs(name):
    with open(os.path.join(TXT, name)) as f:
        return [Fraction(t) for t in f.read().replace(",", " ").split()]


def to_raw(vals, F):
    out = []
    for v in vals:
        r = v * (1 << F)
        assert r.denominator == 1, "golden value %s is not a multiple of 2^-%d" % (v, F)
        out.append(int(r))
    return np.array(out, dtype=np.int64)


def two_tone(fmt, n=1024):
    """Stimulus of the reference FIR testbenches (tests/rtest_ac_fir_const_coeffs.cpp:126-151)."""
    mx = ((1 << (fmt.W - 1)) - 1) / 2.0 ** (fmt.W - fmt.I)
    v = [math.sin(2 * math.pi * 25 * i / 500) + math.sin(2 * math.pi * 150 * i / 500) for i in range(n)]
    am = max(abs(t) for t in v)
    return np.array([from_double((t / am) * mx, fmt) for t in v], dtype=np.int64)


def sqnr_db(y_raw, F, ref):
    yd = y_raw.astype(np.float64) / 2.0 ** F
    r = np.array([float(t) for t in ref], dtype=np.float64)
    return 10 * math.log10((r ** 2).sum() / ((yd - r) ** 2).sum())


def ofmt(f):
    """engine Fmt -> oracle Fmt (same fields, separate ctypes class)."""
    return OFmt(f.W, f.I, f.S, f.Q, f.O)


def windowed_sinc(n_taps, cutoff, fmt, gain=1.0):
    """Symmetric low-pass (Hamming-windowed sinc) quantised to fmt; returns raw int64 coefficients."""
    m = (n_taps - 1) / 2.0
    k = np.arange(n_taps) - m
    h = np.sinc(2 * cutoff * k) * 2 * cutoff * (0.54 - 0.46 * np.cos(2 * np.pi * np.arange(n_taps) / max(n_taps - 1, 1)))
    h = h / h.sum() * gain
    raw = np.round(h * 2.0 ** (fmt.W - fmt.I)).astype(np.int64)
    raw = (raw + raw[::-1]) // 2  # exact symmetry so that the folded architectures are valid
    lo, hi = -(1 << (fmt.W - 1)), (1 << (fmt.W - 1)) - 1
    return np.clip(raw, lo, hi)


# ---------------------------------------------------------------------------------------------
# HIP-graph parity (tests/test_graph_paths_gpu.py): captured run() calls against the CPU oracle
# ---------------------------------------------------------------------------------------------
def rand_fmt(rng, fmt, shape):
    """uniform raw words over the whole range of fmt"""
    lo = -(1 << (fmt.W - 1)) if fmt.S else 0
    hi = (1 << (fmt.W - 1)) - 1 if fmt.S else (1 << fmt.W) - 1
    return rng.integers(lo, hi + 1, size=shape, dtype=np.int64)


def dev_rows(x, fmt):
    """[rows][n] raw words -> device tensor of fmt's containers whose rows start on 64-byte boundaries and are readable, as zeros, up to
    the next multiple of 64 samples beyond n + 16: the layout every matrix-core kernel takes as it is"""
    import torch
    import ac_dsp_amd as A
    x = np.atleast_2d(x)
    n = x.shape[1]
    buf = torch.zeros((x.shape[0], (n + 16 + 63) // 64 * 64), dtype=A.torch_dtype_for(fmt), device="cuda")
    buf[:, :n] = torch.from_numpy(np.ascontiguousarray(x)).to(buf.dtype)
    return buf[:, :n]


def host_words(y):
    return y.cpu().numpy().astype(np.int64)


class GraphCase:
    """One operator under graph capture.  make() -> a fresh engine handle; run(eng, xd) -> its device output for the device rows xd;
    oracle() -> a fresh stateful callable x (raw words) -> expected raw words; fmt = IN_TYPE; path(eng) -> what the case pins (path / kernel class)."""

    def __init__(self, make, run, oracle, fmt, path):
        self.make, self.run, self.oracle, self.fmt, self.path = make, run, oracle, fmt, path


def graph_replays_match_oracle(case, pre, captured, post, expect_path, n_replays=3, reset_after_pre=False):
    """pre: chunks run eagerly in front of the capture; captured(r) -> the nk chunks replay r consumes (same shapes for every r); post: one more
    eager chunk behind the last replay.  reset_after_pre: the eager calls only prime the handle -- reset() then starts the stream (and the oracle) anew.
    Every eager call of the captured handle runs on the capture stream.  Replay r, the eager twin and the trailing eager call are all compared
    bit for bit with the oracle's continuation of the same stream; the path is pinned for every captured call.  Returns the paths."""
    import torch
    side = torch.cuda.Stream()
    eng, twin, orc = case.make(), case.make(), case.oracle()

    def same(got, want, what):
        got = host_words(got)
        assert got.shape == want.shape, (what, got.shape, want.shape)
        bad = np.argwhere(got != want)
        assert bad.size == 0, "%s: %d words differ from the oracle, first at %s" % (what, len(bad), bad[0])

    for i, c in enumerate(pre):
        want = orc(c)
        with torch.cuda.stream(side):
            got = case.run(eng, dev_rows(c, case.fmt))
        side.synchronize()
        same(got, want, "eager call %d in front of the capture" % i)
        same(case.run(twin, dev_rows(c, case.fmt)), want, "twin, eager call %d" % i)
    if reset_after_pre:
        torch.cuda.synchronize()
        eng.reset()
        twin.reset()
        orc = case.oracle()
    first = captured(0)
    xs = [dev_rows(c, case.fmt) for c in first]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    paths, ys = [], []
    with torch.cuda.graph(g, stream=side):
        for xd in xs:
            ys.append(case.run(eng, xd))
            paths.append(case.path(eng))
    torch.cuda.synchronize()
    assert all(p == expect_path for p in paths), (paths, expect_path)
    for r in range(n_replays):
        chunks = first if r == 0 else captured(r)
        for xd, c in zip(xs, chunks):
            assert c.shape == tuple(xd.shape)
            xd.copy_(torch.from_numpy(np.ascontiguousarray(c)).to(xd.dtype))
        for y in ys:
            y.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for k, c in enumerate(chunks):
            want = orc(c)
            same(ys[k], want, "replay %d, call %d" % (r, k))
            same(case.run(twin, dev_rows(c, case.fmt)), want, "twin, replay %d, call %d" % (r, k))
            assert case.path(twin) == expect_path, (case.path(twin), expect_path)
    want = orc(post)
    with torch.cuda.stream(side):
        got = case.run(eng, dev_rows(post, case.fmt))
    side.synchronize()
    same(got, want, "eager call behind the last replay (host-side bookkeeping drifted during the capture?)")
    same(case.run(twin, dev_rows(post, case.fmt)), want, "twin, trailing eager call")
    return paths


def refused_under_capture(legal, illegal):
    """Inside one capture: legal() (returns its device output), then illegal(), which must raise a RuntimeError that names the graph capture.
    The capture must end cleanly.  Returns (graph, output of the legal call, message)."""
    import torch
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    msg = None
    with torch.cuda.graph(g, stream=torch.cuda.Stream()):
        y = legal()
        try:
            illegal()
        except RuntimeError as e:
            msg = str(e)
    torch.cuda.synchronize()
    assert msg is not None, "the call was accepted under capture"
    assert "graph capture" in msg, msg
    return g, y, msg
