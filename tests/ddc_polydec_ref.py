"""Reference and drivers of the polydec cascade tests (test_ddc_polydec_*.py): OracleCic -> OraclePolyDec with the queue of pending
intermediate words kept HERE -- OraclePolyDec.run drops a trailing partial group instead of queueing it, so the helper hands it whole groups of
DF words and carries the rest to the next call, as the reference's ac_channel would (ac_poly_dec.h:110)."""
import numpy as np

from oracle import OracleCic, OraclePolyDec
from helpers import ofmt, windowed_sinc


def polydec_coeffs(n_taps, df, fmt, cutoff=0.2):
    """A windowed-sinc prototype h of NTAPS*DF taps, re-ordered into the array ac_poly_dec takes: c[tp + NTAPS*df] = h[tp*DF + df]."""
    h = windowed_sinc(n_taps * df, cutoff / df, fmt)
    c = np.empty(n_taps * df, dtype=np.int64)
    for d in range(df):
        c[d * n_taps:(d + 1) * n_taps] = h[d::df]
    return c


def prototype_of(c, n_taps, df):
    """The inverse: h[tp*DF + df] = c[tp + NTAPS*df]."""
    h = np.empty(n_taps * df, dtype=np.int64)
    for d in range(df):
        h[d::df] = c[d * n_taps:(d + 1) * n_taps]
    return h


class PolyDecQueue:
    """OraclePolyDec fed in arbitrary bursts: whole groups go to the oracle, the fewer-than-DF words behind them wait."""

    def __init__(self, n_taps, df, fin, fc, fa, fo, n_ch):
        self.df, self.n_ch = df, n_ch
        self.pd = OraclePolyDec(n_taps, df, ofmt(fin), ofmt(fc), ofmt(fa), ofmt(fo), n_ch=n_ch)
        self.pend = np.zeros((n_ch, 0), dtype=np.int64)

    def run(self, c, u):
        u = np.asarray(u, dtype=np.int64)   # [n_ch][words], possibly none
        w = np.concatenate([self.pend, u], axis=1)
        k = w.shape[1] // self.df * self.df
        self.pend = w[:, k:]
        return self.pd.run(c, w[:, :k]) if k else np.zeros((self.n_ch, 0), dtype=np.int64)


def bounds_of(n, splits):
    b = [0] + list(splits or []) + [n]
    return list(zip(b[:-1], b[1:]))


def oracle_mid(R, M, N, cin, mid, x):
    """the decimator's INT_TYPE words of the whole stream (a linear time-invariant stage: the bursts do not matter)"""
    return OracleCic(False, R, M, N, ofmt(cin), ofmt(mid), n_ch=x.shape[0]).run(x).astype(np.int64)


def oracle_cascade(R, M, N, cin, mid, n_taps, df, fc, fa, fo, c, x, splits=None, u=None):
    """OracleCic -> OraclePolyDec over the bursts `splits` of x; u: the words of oracle_mid, when the caller has them already."""
    n_ch = x.shape[0]
    cic = OracleCic(False, R, M, N, ofmt(cin), ofmt(mid), n_ch=n_ch)
    q = PolyDecQueue(n_taps, df, mid, fc, fa, fo, n_ch)
    if u is not None:
        return q.run(c, u)
    outs = [q.run(c, cic.run(x[:, a:b]).astype(np.int64)) if b > a else np.zeros((n_ch, 0), dtype=np.int64) for a, b in bounds_of(x.shape[1], splits)]
    return np.concatenate(outs, axis=1)


def run_stream(ddc, x, splits=None, counts=None, pad=False):
    """the bursts through a DdcPolyDec (or anything with its run()); counts: list that receives the outputs of every burst; pad: every burst in
    rows readable up to a whole 16-sample slot, which the fused kernel asks for (bursts of any length then reach it)"""
    import torch
    outs = []
    for a, b in bounds_of(x.shape[1], splits):
        xd = torch.from_numpy(x[:, a:b].copy()).to(ddc.in_dtype).cuda()
        if pad:
            rows = torch.zeros((x.shape[0], (b - a + 15) // 16 * 16), dtype=ddc.in_dtype, device="cuda")
            rows[:, :b - a] = xd
            xd = rows[:, :b - a]
        y = ddc.run(xd).cpu().numpy().astype(np.int64)
        if counts is not None:
            counts.append(y.shape[1])
        outs.append(y)
    return np.concatenate(outs, axis=1)
