"""CPU-side checks of the polydec cascade (acdsp_ddc_create_polydec): the ABI declares it, the prototype mapping the fused kernel plans with
holds on the oracle, and the queueing of the test helper (ddc_polydec_ref.py) equals a single-call oracle run.  No GPU."""
import os
import re

import numpy as np
import pytest

from oracle import OracleFir, OraclePolyDec, Fmt as OFmt
from ddc_polydec_ref import PolyDecQueue, polydec_coeffs, prototype_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("acdsp_ddc_create_polydec", "acdsp_node_ddc_create_polydec")


def test_header_and_symbol_table_have_the_polydec_cascade():
    import ac_dsp_amd as A
    import ac_dsp_amd._lib as L
    src = open(os.path.join(ROOT, "include", "acdsp.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), "%s is not declared in include/acdsp.h" % name
        assert name in L.SYMBOLS and hasattr(L.lib, name)
    assert issubclass(A.DdcPolyDec, A.Ddc) and issubclass(A.NodeDdcPolyDec, A.NodeDdc)
    assert A.DdcPolyDec._c == "ddc"
    eng = open(os.path.join(ROOT, "include", "ac_dsp", "acdsp_engine.h")).read()
    assert "ddc_polydec_engine" in eng and "acdsp_ddc_create_polydec" in eng


@pytest.mark.parametrize("df", [2, 3, 4])
def test_polydec_is_the_prototype_fir_taken_every_df_th_output(df):
    """h[tp*DF + df] = c[tp + NTAPS*df]: ac_poly_dec on c equals the FIR h on the same words, outputs DF-1, 2DF-1, ... -- bit for bit, with a
    rounding, saturating OUT_TYPE behind an exact-sum accumulator"""
    n_taps = 16
    fin, fc, fa, fo = OFmt(36, 21), OFmt(16, 1), OFmt(60, 30), OFmt(24, 9, True, 1, 1)   # Q = AC_RND, O = AC_SAT
    rng = np.random.default_rng(df)
    c = rng.integers(-32768, 32768, size=n_taps * df)
    x = rng.integers(-(1 << 35), 1 << 35, size=(2, df * 257))
    y = OraclePolyDec(n_taps, df, fin, fc, fa, fo, n_ch=2).run(c, x)
    h = prototype_of(c, n_taps, df)
    z = OracleFir(n_taps * df, "SHIFT_REG", fin, fc, fa, fo, n_ch=2).run(h, x)
    assert y.shape == (2, 257) and np.array_equal(y, np.asarray(z[:, df - 1::df], dtype=np.int64))


def test_the_helper_queues_what_the_oracle_drops():
    """OraclePolyDec.run drops a trailing partial group; fed through PolyDecQueue in bursts of any length the stream equals one call on all of it"""
    n_taps, df = 8, 3
    fin, fc, fa, fo = OFmt(36, 21), OFmt(16, 1), OFmt(60, 30), OFmt(24, 9, True, 1, 1)
    rng = np.random.default_rng(7)
    c = rng.integers(-32768, 32768, size=n_taps * df)
    u = rng.integers(-(1 << 35), 1 << 35, size=(2, 3 * 400 + 2))
    whole = OraclePolyDec(n_taps, df, fin, fc, fa, fo, n_ch=2).run(c, u)
    assert whole.shape == (2, 400)
    # the oracle alone loses a word at a 501 / rest split ...
    o = OraclePolyDec(n_taps, df, fin, fc, fa, fo, n_ch=2)
    lossy = np.concatenate([o.run(c, u[:, :500]), o.run(c, u[:, 500:])], axis=1)
    assert lossy.shape[1] == 166 + 234 and not np.array_equal(lossy, whole)
    # ... the helper does not, whatever the bursts: 2 wait, one word completes their group, a burst without output, an empty one
    from ac_dsp_amd import Fmt
    q = PolyDecQueue(n_taps, df, Fmt(36, 21), Fmt(16, 1), Fmt(60, 30), Fmt(24, 9, True, "RND", "SAT"), 2)
    cuts = [0, 500, 501, 502, 502, 1000, u.shape[1]]
    outs = [q.run(c, u[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    assert [y.shape[1] for y in outs] == [166, 1, 0, 0, 166, 67]
    assert np.array_equal(np.concatenate(outs, axis=1), whole) and q.pend.shape[1] == 2
