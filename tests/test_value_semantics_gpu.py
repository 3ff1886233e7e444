"""GPU tests of the value semantics of every stateful operator family: state blobs (checkpoint / resume) of ac_poly_dec, ac_poly_intr and
ac_intg_dump, and clone() of all seven handle classes.  Everything is bit-exact against the CPU oracle.

The pattern of every case (value_case): one handle runs the whole input and is checked against the oracle; a second handle runs the head,
its blob is restored into a FRESH handle that runs the tail, and the concatenation must equal the whole run; separately a handle is cloned
after the head, original and clone get different tails, in both orders, and each must match the oracle run on its own whole sequence."""
import numpy as np
import pytest
import torch

import ac_dsp_amd as A
from oracle import OraclePolyDec, OraclePolyIntr, OracleIntgDump, OracleMvAvg, OracleCic, OracleFir
from helpers import ofmt, rand_fmt, dev_rows, host_words, windowed_sinc

pytestmark = pytest.mark.gpu

EINVAL = 1
F16 = A.Fmt(16, 2)
FA40 = A.Fmt(40, 12)                        # F = 28 = F_in + F_coeff: exact sums
FA48 = A.Fmt(48, 20)
FO = A.Fmt(16, 10, True, "RND", "SAT")


def same(y, yo, what):
    assert y.shape == yo.shape, (what, y.shape, yo.shape)
    bad = np.argwhere(y != yo)
    assert bad.size == 0, "%s: %d words differ, first at %s: got %d want %d" % (what, len(bad), bad[0], y[tuple(bad[0])], yo[tuple(bad[0])])


class Family:
    """One operator family for value_case.  make(**kw) -> a fresh handle with its coefficients; run(eng, piece) -> raw outputs (numpy);
    oracle() -> a fresh stateful callable piece -> raw outputs; join(p, q) -> the piece that is p followed by q."""

    def __init__(self, make, run, oracle, join=None):
        self.make, self.run, self.oracle = make, run, oracle
        self.join = join or (lambda p, q: np.concatenate([p, q], axis=1))


def value_case(fam, head, tail_a, tail_b, path=None, restore=None, restore_path=None, after_restore=None, checkpoint=True):
    """restore(): the handle the blob is loaded into (default fam.make()); path / restore_path: pinned on the saving and the restoring
    handle, before and after set_state; after_restore(handle): further checks on the restored handle before it runs; checkpoint=False:
    the clone part only."""
    cat = lambda ys: np.concatenate(ys, axis=1)
    whole_a, whole_b = fam.join(head, tail_a), fam.join(head, tail_b)
    want_a, want_b = fam.oracle()(whole_a), fam.oracle()(whole_b)
    # 1. the whole input through one handle
    eng = fam.make()
    y_all = fam.run(eng, whole_a)
    same(y_all, want_a, "one handle, whole input")
    eng.close()
    # 5. clone after the head; different tails; both orders (first, so that the uninterrupted path of the tail call is known below)
    tail_path = None
    for first in ("original", "clone"):
        a = fam.make()
        ya = [fam.run(a, head)]
        if path:
            assert a.path == path, (a.path, path)
        b = a.clone()
        assert type(b) is type(a) and b._h.value != a._h.value
        yb = list(ya)
        if first == "original":
            ya.append(fam.run(a, tail_a)); yb.append(fam.run(b, tail_b))
        else:
            yb.append(fam.run(b, tail_b)); ya.append(fam.run(a, tail_a))
        same(cat(ya), want_a, "original, %s ran first" % first)
        same(cat(yb), want_b, "clone, %s ran first" % first)
        tail_path = a.path
        if path:
            assert a.path == path and b.path == path, (a.path, b.path, path)
        a.close(); b.close()
    if not checkpoint:
        return
    # 2. - 4. head, blob, close; a fresh handle takes the blob and the tail
    a = fam.make()
    y_head = fam.run(a, head)
    if path:
        assert a.path == path, (a.path, path)
    blob = a.state()
    a.close()
    r = (restore or fam.make)()
    r.set_state(blob)
    if after_restore:
        after_restore(r)
    y_tail = fam.run(r, tail_a)
    same(cat([y_head, y_tail]), y_all, "head + restored tail against the whole run")
    assert r.path == (restore_path or tail_path), (r.path, restore_path, tail_path)
    assert r.state()[64:] == fam_state_after(fam, whole_a)[64:], "the restored stream ends in another state than the uninterrupted one"
    r.close()


def fam_state_after(fam, piece):
    eng = fam.make()
    fam.run(eng, piece)
    blob = eng.state()
    eng.close()
    return blob


def refuses(eng, blob, what):
    with pytest.raises(A.AcdspError) as e:
        eng.set_state(blob)
    assert e.value.code == EINVAL, (what, e.value.code, str(e.value))


def refusal_case(fam, head, tail, foreign):
    """foreign: {what: blob} of handles whose blobs this one must refuse; plus a truncated and a corrupted blob of its own.  After every refusal
    the stream is unchanged: the state reads back as before, and the tail still matches the oracle."""
    want = fam.oracle()(fam.join(head, tail))
    eng = fam.make()
    y = [fam.run(eng, head)]
    mine = eng.state()
    bad = dict(foreign)
    bad["truncated"] = mine[:-8]
    bad["header only"] = mine[:64]
    bad["shorter than a header"] = mine[:40]
    bad["one byte too long"] = mine + b"\0"
    bad["corrupted magic"] = b"X" + mine[1:]
    for what, blob in bad.items():
        refuses(eng, blob, what)
        assert eng.state() == mine, what
    y.append(fam.run(eng, tail))
    same(np.concatenate(y, axis=1), want, "after the refusals")
    eng.close()


def blob_of(eng):
    b = eng.state()
    eng.close()
    return b


# ---------------------------------------------------------------------------------------------
# ac_poly_dec
# ---------------------------------------------------------------------------------------------
def polydec_family(nt, df, n_ch, fa=FA40, seed=1, **kw0):
    c = np.random.default_rng(seed).integers(-32768, 32640, size=nt * df, dtype=np.int64)

    def make(**kw):
        args = dict(kw0)
        args.update(kw)
        eng = A.PolyDec(nt, df, F16, F16, fa, FO, n_channels=n_ch, **args)
        eng.set_coeffs(c)
        return eng

    def run(eng, x):
        return host_words(eng.run(dev_rows(x, F16)))

    def oracle():
        orc = OraclePolyDec(nt, df, ofmt(F16), ofmt(F16), ofmt(fa), ofmt(FO), n_ch=n_ch)
        return lambda x: orc.run(c, x)

    return Family(make, run, oracle)


def polydec_pieces(df, n_ch, n_groups, seed=2):
    """cut = DF * 333: a number of groups that is no multiple of 16"""
    rng = np.random.default_rng(seed)
    x = rand_fmt(rng, F16, (n_ch, n_groups * df))
    cut = df * 333
    return x[:, :cut], x[:, cut:], rand_fmt(rng, F16, (n_ch, (n_groups - 333 - 7) * df))


@pytest.mark.parametrize("force_generic,path", [(False, "mfma_gen"), (True, "generic")])
def test_polydec_checkpoint_and_clone(force_generic, path):
    fam = polydec_family(8, 4, 5, force_generic=force_generic)
    value_case(fam, *polydec_pieces(4, 5, 700), path=path)


@pytest.mark.parametrize("from_generic", [False, True])
def test_polydec_blob_crosses_the_kernel_paths(from_generic):
    fam = polydec_family(8, 4, 5, force_generic=from_generic)
    value_case(fam, *polydec_pieces(4, 5, 700), path="generic" if from_generic else "mfma_gen",
               restore=lambda: fam.make(force_generic=not from_generic), restore_path="mfma_gen" if from_generic else "generic")


def test_polydec_long_checkpoint_clone_and_another_scratch_cap():
    fam = polydec_family(129, 16, 2, fa=FA48)
    head, tail_a, tail_b = polydec_pieces(16, 2, 1500)

    def restore():
        r = fam.make()
        r.set_scratch_cap(1 << 16)          # below the floor of 8 channels x 1024 outputs: the smallest geometry
        return r

    value_case(fam, head, tail_a, tail_b, path="mfma_long", restore=restore)
    a = fam.make()
    a.set_scratch_cap(1 << 16)
    b = a.clone()
    assert b.long_geometry() == a.long_geometry() != fam.make().long_geometry()   # the clone keeps the cap


def test_polydec_refusals():
    fam = polydec_family(8, 4, 5)
    head, tail, _ = polydec_pieces(4, 5, 400)
    intr = polyintr_family(16, 4, "FOLD_EVEN", 5)
    refusal_case(fam, head, tail, {
        "another family": blob_of(intr.make()),
        "another NTAPS": blob_of(polydec_family(7, 4, 5).make()),
        "another DF": blob_of(polydec_family(8, 2, 5).make()),
        "another channel count": blob_of(polydec_family(8, 4, 4).make()),
    })


# ---------------------------------------------------------------------------------------------
# ac_poly_intr
# ---------------------------------------------------------------------------------------------
def table_size(n_taps, ifac, ftype):
    j = ifac - 1
    return {"FOLD_EVEN": (n_taps // 2 - 1) + j * n_taps // 2, "FOLD_ODD": (n_taps - 1) // 2 + (n_taps // 2 + 1) * j,
            "FOLD_ANTI": (n_taps - 1) + n_taps * j}[ftype] + 1


def polyintr_family(n_taps, ifac, ftype, n_ch, fa=FA40, seed=3, long_set=False, **kw0):
    rng = np.random.default_rng(seed)
    if long_set:       # what the long kernels take: every sign set, pair differences that split into two signed bytes
        csz = table_size(n_taps, ifac, ftype)
        c, sign = rng.integers(-16000, 16000, size=csz, dtype=np.int64), np.ones(ifac, dtype=np.int64)
    else:              # the control words of the family's own parity tests: COEFFSZ beyond what the loops read, random signs
        csz = table_size(n_taps, ifac, ftype) + 2
        c, sign = rand_fmt(rng, F16, (csz,)), rng.integers(0, 2, size=ifac)
    corr = ifac - 1 - np.arange(ifac)      # symmetric pairs

    def make(**kw):
        args = dict(kw0)
        args.update(kw)
        eng = A.PolyIntr(n_taps, csz, ifac, ftype, F16, F16, fa, FO, n_channels=n_ch, **args)
        eng.set_ctrl(c, sign, corr)
        return eng

    def run(eng, x):
        return host_words(eng.run(dev_rows(x, F16)))

    def oracle():
        orc = OraclePolyIntr(n_taps, csz, ifac, ftype, ofmt(F16), ofmt(F16), ofmt(fa), ofmt(FO), n_ch=n_ch)
        return lambda x: orc.run(c, sign, corr, x)

    return Family(make, run, oracle)


def polyintr_pieces(n_ch, cut, n, seed=4):
    rng = np.random.default_rng(seed)
    x = rand_fmt(rng, F16, (n_ch, n))
    return x[:, :cut], x[:, cut:], rand_fmt(rng, F16, (n_ch, n - cut - 9))


def counts_like_a_started_stream(ifac, ftype, cut):
    def check(r):
        # the folded cores emit nothing for a stream's first sample only: the restored handle is `cut` samples in
        assert r.out_count(5) == 5 * ifac, (r.out_count(5), ftype, cut)
    return check


@pytest.mark.parametrize("force_generic", [False, True])
@pytest.mark.parametrize("cut", [1, 257])
@pytest.mark.parametrize("ftype", ["FOLD_EVEN", "FOLD_ODD", "FOLD_ANTI"])
def test_polyintr_checkpoint_and_clone(ftype, cut, force_generic):
    fam = polyintr_family(16, 4, ftype, 5, force_generic=force_generic)
    value_case(fam, *polyintr_pieces(5, cut, 700), after_restore=counts_like_a_started_stream(4, ftype, cut))


@pytest.mark.parametrize("from_generic", [False, True])
@pytest.mark.parametrize("cut", [1, 257])
def test_polyintr_blob_crosses_the_kernel_paths(cut, from_generic):
    fam = polyintr_family(16, 4, "FOLD_EVEN", 5, force_generic=from_generic)
    fast = fam.make(force_generic=False)
    fam.run(fast, polyintr_pieces(5, cut, 700)[1])
    fast_path = fast.path
    assert fast_path != "generic"
    value_case(fam, *polyintr_pieces(5, cut, 700), restore=lambda: fam.make(force_generic=not from_generic),
               restore_path=fast_path if from_generic else "generic", after_restore=counts_like_a_started_stream(4, "FOLD_EVEN", cut))


def test_polyintr_long_checkpoint_and_clone():
    fam = polyintr_family(80, 3, "FOLD_EVEN", 2, fa=FA48, long_set=True)
    value_case(fam, *polyintr_pieces(2, 700, 2000), path="mfma_long", after_restore=counts_like_a_started_stream(3, "FOLD_EVEN", 700))


def test_polyintr_refusals():
    fam = polyintr_family(16, 4, "FOLD_EVEN", 5)
    head, tail, _ = polyintr_pieces(5, 257, 500)
    refusal_case(fam, head, tail, {
        "another family": blob_of(polydec_family(8, 4, 5).make()),
        "another NTAPS": blob_of(polyintr_family(14, 4, "FOLD_EVEN", 5).make()),
        "another IF": blob_of(polyintr_family(16, 3, "FOLD_EVEN", 5).make()),
        "another ftype": blob_of(polyintr_family(16, 4, "FOLD_ANTI", 5).make()),
        "another channel count": blob_of(polyintr_family(16, 4, "FOLD_EVEN", 6).make()),
    })


# ---------------------------------------------------------------------------------------------
# ac_intg_dump: a piece is (rows of samples, n_sample table)
# ---------------------------------------------------------------------------------------------
def intgdump_family(ns, chn, n_obj, fin, fa, fo):
    def make():
        return A.IntgDump(ns, chn, fin, fa, fo, n_objects=n_obj)

    def run(eng, piece):
        x, table = piece
        return host_words(eng.run(dev_rows(x, fin), table))

    def oracle():
        orc = OracleIntgDump(ns, chn, ofmt(fin), ofmt(fa), ofmt(fo), n_obj=n_obj)
        return lambda piece: orc.run(piece[0], piece[1])

    def join(p, q):
        return np.concatenate([p[0], q[0]], axis=1), list(p[1]) + list(q[1])

    return Family(make, run, oracle, join)


def intgdump_pieces(ns, chn, n_obj, fin, tables, seed=5):
    rng = np.random.default_rng(seed)
    out = []
    for t in tables:
        rounds = sum(v if 1 <= v <= ns else ns for v in t)
        out.append((rand_fmt(rng, fin, (n_obj, rounds * chn)), list(t)))
    return out


# the head ends on n_sample = 0: NS rounds, no dump, the sums carry over the cut.  Every block of the first tail dumps: a handle that
# forgot that sums are pending would take a kernel that never looks at temp[].  The second tail carries sums a second time.
PENDING = ([5, 16, 3, 0], [4, 16, 7, 2], [1, 0, 9, 20, 3])
ALL_DUMP = ([16] * 6, [16] * 5, [16] * 7)                     # every block dumps: nothing is pending at the cut


@pytest.mark.parametrize("tables", [PENDING, ALL_DUMP], ids=["pending_at_the_cut", "every_block_dumps"])
@pytest.mark.parametrize("chn", [3, 7])
def test_intgdump_checkpoint_and_clone(chn, tables):
    fin, fa = A.Fmt(16, 8), A.Fmt(32, 16)
    fam = intgdump_family(16, chn, 5, fin, fa, fa)
    value_case(fam, *intgdump_pieces(16, chn, 5, fin, tables))


def test_intgdump_saturating_accumulator_on_the_exact_order_kernel():
    # fewer fraction bits than the input and AC_SAT: every add quantises and may saturate, the carried sums included
    fin, fa, fo = A.Fmt(16, 4), A.Fmt(18, 8, True, "RND", "SAT"), A.Fmt(10, 7, True, "RND", "SAT")
    fam = intgdump_family(16, 3, 5, fin, fa, fo)
    value_case(fam, *intgdump_pieces(16, 3, 5, fin, PENDING), path="exact_order")


def test_intgdump_refusals():
    fin, fa = A.Fmt(16, 8), A.Fmt(32, 16)
    fam = intgdump_family(16, 3, 5, fin, fa, fa)
    head, tail, _ = intgdump_pieces(16, 3, 5, fin, PENDING)
    refusal_case(fam, head, tail, {
        "another family": blob_of(polydec_family(8, 4, 5).make()),
        "another CHN": blob_of(intgdump_family(16, 7, 5, fin, fa, fa).make()),
        "another NS": blob_of(intgdump_family(8, 3, 5, fin, fa, fa).make()),
        "another object count": blob_of(intgdump_family(16, 3, 4, fin, fa, fa).make()),
    })


# ---------------------------------------------------------------------------------------------
# ac_mv_avg and the DDC cascade: clone() only
# ---------------------------------------------------------------------------------------------
def test_mvavg_clone_gives_the_same_frames():
    fin, fc, fa, fo = F16, A.Fmt(16, 1), FA40, FO
    rng = np.random.default_rng(6)
    c = rand_fmt(rng, fc, (17,))
    x = rand_fmt(rng, fin, (3, 4 * 50))
    want = OracleMvAvg(17, "MIRROR", ofmt(fin), ofmt(fc), ofmt(fa), ofmt(fo), n_obj=3).run(c, x, 50)
    a = A.MvAvg(64, 17, "MIRROR", fin, fc, fa, fo, n_objects=3)
    early = a.clone()                        # before the coefficients are bound: the clone takes its own
    a.set_coeffs(c)
    ya = host_words(a.run(dev_rows(x, fin), 50))
    b = a.clone()
    assert type(b) is A.MvAvg and b._h.value != a._h.value
    a.close()
    yb = host_words(b.run(dev_rows(x, fin), 50))
    same(ya, want, "original")
    same(yb, want, "clone, original closed")
    with pytest.raises(A.AcdspError):
        early.run(dev_rows(x, fin), 50)
    early.set_coeffs(c)
    same(host_words(early.run(dev_rows(x, fin), 50)), want, "clone of a handle without coefficients")


def ddc_family(R, cin, n_taps, fc, fa, fo, n_ch):
    c = windowed_sinc(n_taps, 0.2, fc)
    probe = A.Ddc(R, 1, 5, cin, n_taps, "SHIFT_REG", fc, fa, fo, n_channels=n_ch)
    mid = probe.int_type
    probe.close()

    def make():
        eng = A.Ddc(R, 1, 5, cin, n_taps, "SHIFT_REG", fc, fa, fo, n_channels=n_ch)
        eng.set_coeffs(c)
        return eng

    def run(eng, x):
        return host_words(eng.run(dev_rows(x, cin)))

    def oracle():
        cic = OracleCic(False, R, 1, 5, ofmt(cin), ofmt(mid), n_ch=n_ch)
        fir = OracleFir(n_taps, "SHIFT_REG", ofmt(mid), ofmt(fc), ofmt(fa), ofmt(fo), n_ch=n_ch)
        return lambda x: fir.run(c, cic.run(x))

    return Family(make, run, oracle)


@pytest.mark.parametrize("shape,path", [
    (dict(R=16, cin=A.Fmt(16, 1), n_taps=127, fc=A.Fmt(16, 1), fa=A.Fmt(60, 30), fo=A.Fmt(24, 9, True, "RND", "SAT"), n_ch=3), "fused"),
    (dict(R=8, cin=A.Fmt(32, 16), n_taps=63, fc=A.Fmt(16, 1), fa=A.Fmt(64, 31), fo=A.Fmt(32, 16, True, "RND", "SAT"), n_ch=2), "two_kernels"),
])
def test_ddc_clone_carries_both_stages(shape, path):
    fam = ddc_family(**shape)
    rng = np.random.default_rng(7)
    R, n_ch = shape["R"], shape["n_ch"]
    x = rand_fmt(rng, shape["cin"], (n_ch, R * 900 + 5))
    cut = R * 400 + 3                        # the cut stands inside a decimation period: the phase goes with the clone
    # (the cascade's blobs have their own tests in test_ddc_gpu.py: the clone part only)
    value_case(fam, x[:, :cut], x[:, cut:], rand_fmt(rng, shape["cin"], (n_ch, R * 300 + 1)), path=path, checkpoint=False)


def test_fir_and_cic_handles_clone_from_python():
    rng = np.random.default_rng(8)
    c = rand_fmt(rng, F16, (31,))
    x = rand_fmt(rng, F16, (3, 900))
    fir = A.Fir(31, "SHIFT_REG", F16, F16, FA40, FO, n_channels=3)
    fir.set_coeffs(c)
    y0 = host_words(fir.run(dev_rows(x[:, :333], F16)))
    twin = fir.clone()
    assert type(twin) is A.Fir and twin.path == fir.path
    want = OracleFir(31, "SHIFT_REG", ofmt(F16), ofmt(F16), ofmt(FA40), ofmt(FO), n_ch=3).run(c, x)
    same(np.concatenate([y0, host_words(twin.run(dev_rows(x[:, 333:], F16)))], axis=1), want, "FIR clone")
    same(np.concatenate([y0, host_words(fir.run(dev_rows(x[:, 333:], F16)))], axis=1), want, "FIR original")
    cin, cout = A.Fmt(16, 8), A.Fmt(31, 23)
    cic = A.Cic(False, 8, 1, 5, cin, cout, n_channels=3)
    y0 = host_words(cic.run(dev_rows(x[:, :333], cin)))
    twin = cic.clone()
    assert type(twin) is A.Cic
    want = OracleCic(False, 8, 1, 5, ofmt(cin), ofmt(cout), n_ch=3).run(x)
    same(np.concatenate([y0, host_words(twin.run(dev_rows(x[:, 333:], cin)))], axis=1), want, "CIC clone")
    same(np.concatenate([y0, host_words(cic.run(dev_rows(x[:, 333:], cin)))], axis=1), want, "CIC original")


# ---------------------------------------------------------------------------------------------
# input-history blobs of another history length (the rule of acdsp_fir_state_set): taken when they cover the filter memory
# ---------------------------------------------------------------------------------------------
def relen_blob(blob, new_len, rng):
    """the blob of an input-history family with `new_len` samples per channel: the newest ones kept, older ones filled with noise (a
    longer history holds samples from before the filter memory); what follows the histories stays"""
    import struct
    hdr = list(struct.unpack("<8sIIIIQq4IQ", blob[:64]))
    n_ch, eb, per = hdr[3], hdr[4], hdr[5]
    assert eb == 2
    hist = np.frombuffer(blob[64:64 + n_ch * per * eb], dtype=np.int16).reshape(n_ch, per)
    out = rng.integers(-32768, 32768, size=(n_ch, new_len)).astype(np.int16)
    keep = min(per, new_len)
    out[:, new_len - keep:] = hist[:, per - keep:]
    hdr[5] = new_len
    return struct.pack("<8sIIIIQq4IQ", *hdr) + out.tobytes() + blob[64 + n_ch * per * eb:]


CIC_IN, CIC_OUT = A.Fmt(16, 8), A.Fmt(31, 23)


def cic_family(interp, n_ch, R=8, M=1, N=5):
    def make():
        return A.Cic(interp, R, M, N, CIC_IN, CIC_OUT, n_channels=n_ch)

    def run(eng, x):
        return host_words(eng.run(dev_rows(x, CIC_IN)))

    def oracle():
        orc = OracleCic(interp, R, M, N, ofmt(CIC_IN), ofmt(CIC_OUT), n_ch=n_ch)
        return orc.run

    return Family(make, run, oracle)


def cic_pieces(n_ch, seed=10):
    """a head of 333 samples: no multiple of R = 8, the decimation phase goes with the blob"""
    x = rand_fmt(np.random.default_rng(seed), CIC_IN, (n_ch, 900))
    return x[:, :333], x[:, 333:], None


def fir_family(n_taps, ftype, n_ch, kind="load", seed=11):
    c = rand_fmt(np.random.default_rng(seed), F16, (n_taps,))

    def make():
        eng = A.Fir(n_taps, ftype, F16, F16, FA40, FO, n_channels=n_ch, kind=kind)
        eng.set_coeffs(c)
        return eng

    def run(eng, x):
        return host_words(eng.run(dev_rows(x, F16)))

    def oracle():
        orc = OracleFir(n_taps, ftype, ofmt(F16), ofmt(F16), ofmt(FA40), ofmt(FO), n_ch=n_ch)
        return lambda x: orc.run(c, x)

    return Family(make, run, oracle)


def blob_per_channel(blob):
    import struct
    return struct.unpack("<8sIIIIQq4IQ", blob[:64])[5]


@pytest.mark.parametrize("family", ["polydec", "polyintr", "cic_dec", "cic_intr"])
def test_history_blobs_of_another_length(family):
    own = None                   # (CIC: read from the blob -- a handle that takes the two-stage kernel keeps a longer history)
    if family == "polydec":      # NTAPS*DF = 32: an output reaches 31 samples back, the handle keeps 64
        fam, (head, tail, _), mem, own = polydec_family(8, 4, 5), polydec_pieces(4, 5, 700), 31, 64
    elif family == "polyintr":   # NTAPS = 16: the sums of a call's first group reach 16 samples back, the handle keeps 32
        fam, (head, tail, _), mem, own = polyintr_family(16, 4, "FOLD_EVEN", 5), polyintr_pieces(5, 257, 700), 16, 32
    elif family == "cic_dec":    # R = 8, M = 1, N = 5: the filter memory is N R M - 1 = 39 inputs
        fam, (head, tail, _), mem = cic_family(False, 4), cic_pieces(4), 39
    else:                        # the interpolator's memory: N M + 1 = 6 inputs
        fam, (head, tail, _), mem = cic_family(True, 4), cic_pieces(4), 6
    rng = np.random.default_rng(9)
    want = fam.oracle()(fam.join(head, tail))
    a = fam.make()
    y_head = fam.run(a, head)
    blob = blob_of(a)
    if own is None:
        own = blob_per_channel(blob)
        assert own > mem
    assert len(relen_blob(blob, own, rng)) == len(blob)
    for new_len in (own + 32, mem):
        r = fam.make()
        r.set_state(relen_blob(blob, new_len, rng))
        same(np.concatenate([y_head, fam.run(r, tail)], axis=1), want, "history of %d samples" % new_len)
        r.close()
    r = fam.make()
    mine = r.state()
    refuses(r, relen_blob(blob, mem - 1, rng), "a history shorter than the filter memory")
    refuses(r, relen_blob(blob, own + 32, rng)[:-2], "a longer history, truncated")
    assert r.state() == mine


def test_fir_reg_trans_blob_of_another_length_is_refused():
    """TRANSPOSED with loadable coefficients carries reg_trans partial sums (a kind-2 blob): no other length is this filter's state"""
    import struct
    fam = fir_family(40, "TRANSPOSED", 2)
    eng = fam.make()
    fam.run(eng, rand_fmt(np.random.default_rng(12), F16, (2, 300)))
    mine = eng.state()
    hdr = list(struct.unpack("<8sIIIIQq4IQ", mine[:64]))
    assert hdr[2] == 2 and hdr[3] == 2 and hdr[5] == 40, hdr          # kind 2, 2 channels, n_taps words per channel
    hdr[5] = 41
    longer = struct.pack("<8sIIIIQq4IQ", *hdr) + mine[64:] + bytes(2 * hdr[4])
    assert len(longer) == 64 + 2 * 41 * hdr[4]
    refuses(eng, longer, "reg_trans words of another length")
    assert eng.state() == mine
    eng.close()


def stateful_families():
    fin, fa = A.Fmt(16, 8), A.Fmt(32, 16)
    return {
        "fir": fir_family(31, "SHIFT_REG", 3),
        "cic": cic_family(False, 4),
        "ddc": ddc_family(R=16, cin=A.Fmt(16, 1), n_taps=127, fc=A.Fmt(16, 1), fa=A.Fmt(60, 30), fo=A.Fmt(24, 9, True, "RND", "SAT"), n_ch=3),
        "polydec": polydec_family(8, 4, 5),
        "polyintr": polyintr_family(16, 4, "FOLD_EVEN", 5),
        "intgdump": intgdump_family(16, 3, 5, fin, fa, fa),
    }


@pytest.mark.parametrize("name", ["fir", "cic", "ddc", "polydec", "polyintr", "intgdump"])
def test_state_blob_messages(name):
    import ctypes as C
    eng = stateful_families()[name].make()
    mine = eng.state()
    with pytest.raises(A.AcdspError) as e:
        eng.set_state(mine[:63])
    assert e.value.code == EINVAL and str(e.value).endswith("%s_state_set: blob shorter than its header" % name), str(e.value)
    size = getattr(A.lib, "acdsp_%s_state_size" % name)(eng._h)
    assert size == len(mine)
    buf = (C.c_char * size)()
    assert getattr(A.lib, "acdsp_%s_state_get" % name)(eng._h, buf, size - 1) == EINVAL
    msg = A.lib.acdsp_last_error().decode()
    assert msg.startswith("%s_state_get: buffer of %d bytes" % (name, size - 1)) and "state needs %d" % size in msg, msg
    assert eng.state() == mine
    eng.close()
