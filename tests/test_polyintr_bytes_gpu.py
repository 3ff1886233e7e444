"""GPU tests of byte rows on ac_poly_intr: PolyIntr(in_bytes=True[, out_bytes=True]) = ACDSP_FLAG_IN_BYTES [| ACDSP_FLAG_OUT_BYTES].  int8 /
uint8 input rows, 1-byte or int16 output rows, on the interpolating matrix-core kernel with one sample plane (fir_up_s8.hip, path "mfma_gen")
and on the exact VALU kernels beside it.  Every value is compared for equality with OraclePolyIntr on the same raw words (the oracle knows no
containers); some cases also with an unflagged handle on int16 containers of the same values.

Types: COEFF <16,2> full range, IN <8,2>, ACC <32,12> (F_acc = F_in + F_coeff: the 32-bit epilogue; 16 taps bound |sum| by 2^28 even for pair
sets, 40 taps by 2^30 without pairs).  The matrix-core kernel needs one whole step of 512 samples behind 2 NB slots of 16: calls of at least
544 (one K block) / 576 (two) samples.  The parity stream of 3401 samples is cut into calls of 1 (emits nothing on the folded cores), 700 (one
step) and 2700 samples (five steps = a four-step wave and a one-step wave at IF 2, and a 108-sample tail on the VALU kernels)."""
import numpy as np
import pytest
import torch

import ac_dsp_amd as A
from oracle import OracleFir, OraclePolyIntr
from helpers import ofmt, rand_fmt

pytestmark = pytest.mark.gpu

F = A.Fmt
FIN, FC, FA = F(8, 2), F(16, 2), F(32, 12)
FO8, FO16 = F(8, 2, True, "RND", "SAT"), F(16, 2, True, "RND", "SAT")
CORES = [("FOLD_EVEN", 16), ("FOLD_ODD", 15), ("FOLD_ANTI", 12)]
SPLITS = [1, 701]
N = 3401
VALU = ("lossless64", "generic")


def table_size(n_taps, ifac, ftype):
    j = ifac - 1
    return {"FOLD_EVEN": (n_taps // 2 - 1) + j * n_taps // 2, "FOLD_ODD": (n_taps - 1) // 2 + (n_taps // 2 + 1) * j,
            "FOLD_ANTI": (n_taps - 1) + n_taps * j}[ftype] + 1


def np_bytes(fmt):
    return np.int8 if fmt.S else np.uint8


def rows(x, dtype, lead=0):
    """[n_ch][n] raw words -> device rows of `dtype` containers with a pitch that is a multiple of 16 elements, `lead` elements into it"""
    n_ch, n = x.shape
    buf = torch.zeros((n_ch, (lead + n + 15) // 16 * 16 + 16), dtype=dtype, device="cuda")
    buf[:, lead:lead + n] = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
    return buf[:, lead:lead + n]


def out_rows(eng, n_in):
    no = max(eng.out_count(n_in), 1)
    return torch.zeros((eng.n_channels, (no + 15) // 16 * 16 + 16), dtype=eng.out_dtype, device="cuda")[:, :no]


def words(y):
    return y.cpu().numpy().astype(np.int64)


def same(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d words differ, first at %s: got %d want %d" % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def control(rng, n_taps, ifac, ftype, pairs, coeff_bits=16, sign=None):
    csz = table_size(n_taps, ifac, ftype) + 1
    c = rng.integers(-(1 << (coeff_bits - 1)), 1 << (coeff_bits - 1), size=csz, dtype=np.int64)
    sg = np.ones(ifac, dtype=np.int64) if sign is None else np.asarray(sign)
    corr = (ifac - 1 - np.arange(ifac)) if pairs else np.arange(ifac)
    return csz, c, sg, corr


def stimulus(rng, fin, n_ch, n):
    x = rand_fmt(rng, fin, (n_ch, n))
    lo, hi = (-(1 << (fin.W - 1)), (1 << (fin.W - 1)) - 1) if fin.S else (0, (1 << fin.W) - 1)
    x[0, 40:120] = lo                                        # runs of -128 and of 127 across a step's history and its first columns
    x[0, 700:790] = hi
    x[-1, 1200:1300] = lo
    return x


class Case:
    """a flagged handle, the oracle and (twin=True) an unflagged handle on int16 containers, fed the same stream call by call"""

    def __init__(self, n_taps, ifac, ftype, fo, out_bytes, n_ch=3, seed=0, pairs=False, coeff_bits=16, sign=None, fin=FIN, fa=FA, twin=False, **kw):
        self.rng = np.random.default_rng(seed)
        self.fin, self.fo, self.n_ch, self.ifac = fin, fo, n_ch, ifac
        self.csz, self.c, self.sg, self.corr = control(self.rng, n_taps, ifac, ftype, pairs, coeff_bits, sign)
        self.args = (n_taps, self.csz, ifac, ftype, fin, FC, fa, fo)
        self.eng = A.PolyIntr(*self.args, n_channels=n_ch, in_bytes=True, out_bytes=out_bytes, **kw)
        self.eng.set_ctrl(self.c, self.sg, self.corr)
        self.orc = OraclePolyIntr(n_taps, self.csz, ifac, ftype, ofmt(fin), ofmt(FC), ofmt(fa), ofmt(fo), n_ch=n_ch)
        self.twin = None
        if twin:
            self.twin = A.PolyIntr(*self.args, n_channels=n_ch)
            self.twin.set_ctrl(self.c, self.sg, self.corr)
        self.paths = []

    def call(self, x, lead=0, what=""):
        xd = rows(x, self.eng.in_dtype, lead)
        y = self.eng.run(xd, out=out_rows(self.eng, x.shape[1]))
        self.paths.append(self.eng.path)
        assert y.dtype == self.eng.out_dtype
        want = self.orc.run(self.c, self.sg, self.corr, x)
        same(words(y), want, "%s call %d (%s)" % (what, len(self.paths), self.eng.path))
        if self.twin is not None:
            same(words(self.twin.run(rows(x, torch.int16))), want, "%s int16 twin, call %d" % (what, len(self.paths)))
        return y

    def stream(self, x, splits, what=""):
        bounds = [0] + list(splits) + [x.shape[1]]
        for a, b in zip(bounds[:-1], bounds[1:]):
            self.call(x[:, a:b], what=what)
        return self.paths


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_bytes", [True, False], ids=["out1", "out2"])
@pytest.mark.parametrize("ftype,n_taps", CORES)
@pytest.mark.parametrize("ifac", [2, 3, 4, 5, 6, 7, 8, 16])
def test_parity_with_the_oracle_on_the_matrix_cores(ifac, ftype, n_taps, out_bytes):
    fo = FO8 if out_bytes else FO16
    k = Case(n_taps, ifac, ftype, fo, out_bytes, seed=ifac * 31 + n_taps, pairs=True, twin=(ifac == {"FOLD_EVEN": 8, "FOLD_ODD": 5, "FOLD_ANTI": 2}[ftype]))
    assert A._lib.lib.acdsp_polyintr_in_elem_bytes(k.eng._h) == 1 and A._lib.lib.acdsp_polyintr_out_elem_bytes(k.eng._h) == (1 if out_bytes else 2)
    paths = k.stream(stimulus(k.rng, FIN, 3, N), SPLITS)
    assert paths[0] in VALU and paths[1:] == ["mfma_gen", "mfma_gen"], paths
    if ftype == "FOLD_ANTI":
        return
    # a stream that starts with a long call: the folded cores emit its outputs IF containers in front of the row, so with 1-byte rows a factor
    # that is no multiple of 4 (int16 rows: an odd one) leaves THAT call on the VALU kernels; the next call starts on the row again
    k2 = Case(n_taps, ifac, ftype, fo, out_bytes, seed=ifac * 31 + n_taps + 1, pairs=True)
    paths = k2.stream(stimulus(k2.rng, FIN, 3, 1400), [700], what="long first call")
    first_on_grid = (ifac * (1 if out_bytes else 2)) % 4 == 0
    assert (paths[0] == "mfma_gen") == first_on_grid and (first_on_grid or paths[0] in VALU), (paths, ifac)
    assert paths[1] == "mfma_gen", paths


# ---- 2. output types ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fo,fa", [(F(8, 2, True, "RND", "SAT"), FA), (F(8, 2, True, "TRN", "WRAP"), FA), (F(6, 2, True, "RND", "SAT"), FA), (F(8, 3, False, "RND", "SAT"), FA),
                                   (F(5, 1, True, "TRN", "WRAP"), FA), (F(8, 2, True, "RND_CONV", "SAT_SYM"), FA), (F(8, 2, True, "RND", "SAT"), F(40, 12))],
                         ids=["rnd_sat", "trn_wrap", "w6_rnd_sat", "unsigned_rnd_sat", "w5_trn_wrap", "conv_satsym", "acc_shift_8"])
@pytest.mark.parametrize("out_bytes", [True, False], ids=["out1", "out2"])
def test_output_types_on_both_epilogues(fo, fa, out_bytes):
    """the first four run the 32-bit epilogue (AC_TRN / AC_RND into AC_SAT, or AC_WRAP at the container width -- for int16 rows <8,2,TRN,WRAP>
    is the generic one), the others the generic epilogue (F_acc = F_in + F_coeff + 8: a left shift into ACC_TYPE)"""
    for ftype, n_taps, ifac, pairs in (("FOLD_EVEN", 16, 8, True), ("FOLD_ANTI", 12, 2, False)):
        k = Case(n_taps, ifac, ftype, fo, out_bytes, seed=7 + ifac, pairs=pairs, fa=fa)
        paths = k.stream(stimulus(k.rng, FIN, 3, N), SPLITS, what=ftype)
        assert paths[1:] == ["mfma_gen", "mfma_gen"], paths
        assert k.eng.out_dtype == ((torch.int8 if fo.S else torch.uint8) if out_bytes else torch.int16)


# ---- 3. digit planes and K blocks -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_bytes", [True, False], ids=["out1", "out2"])
@pytest.mark.parametrize("shape", ["two_planes", "three_planes_pairs", "two_k_blocks"])
def test_digit_planes_and_k_blocks(shape, out_bytes):
    fo = FO8 if out_bytes else FO16
    if shape == "two_planes":                               # |folded tap| < 2^15: 13-bit coefficients, no pairs
        k = Case(16, 8, "FOLD_EVEN", fo, out_bytes, seed=21, pairs=False, coeff_bits=13)
    elif shape == "three_planes_pairs":                     # corr = IF-1-j, all signs 1: the pair taps E_j - E_cj have 17 bits
        k = Case(16, 4, "FOLD_EVEN", fo, out_bytes, seed=22, pairs=True, coeff_bits=16)
    else:                                                   # 40 taps at IF 4: 8 samples per column + 39 earlier ones = two K blocks
        k = Case(40, 4, "FOLD_ANTI", fo, out_bytes, seed=23, pairs=False, coeff_bits=16)
    paths = k.stream(stimulus(k.rng, FIN, 3, N), SPLITS, what=shape)
    assert paths[1:] == ["mfma_gen", "mfma_gen"], paths


# ---- 4. off the fast path, still exact ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_bytes", [True, False], ids=["out1", "out2"])
def test_off_the_fast_path_the_rows_are_still_exact(out_bytes):
    fo = FO8 if out_bytes else FO16
    # a row pointer one element off the 16-byte grid
    k = Case(16, 4, "FOLD_EVEN", fo, out_bytes, seed=31, pairs=True)
    k.call(stimulus(k.rng, FIN, 3, 700), what="aligned")
    k.call(stimulus(k.rng, FIN, 3, 1400), lead=1, what="one element off")
    k.call(stimulus(k.rng, FIN, 3, 700), what="aligned again")
    assert k.paths[0] == "mfma_gen" and k.paths[1] in VALU and k.paths[2] == "mfma_gen", k.paths
    # a phase with sign[j] = 0 on a folded core negates samples in IN_TYPE (-(-128) wraps): not linear
    k = Case(16, 4, "FOLD_EVEN", fo, out_bytes, seed=32, pairs=True, sign=[1, 0, 1, 1])
    assert set(k.stream(stimulus(k.rng, FIN, 3, 1500), [1, 701], what="sign 0")) == {"lossless64"}
    # unsigned samples: the exact-accumulation class wants a signed IN_TYPE -- exact-order kernel on uint8 rows
    fu = F(8, 8, False)
    k = Case(12, 4, "FOLD_ANTI", F(8, 8, False, "RND", "SAT") if out_bytes else F(16, 12, True, "RND", "SAT"), out_bytes, seed=33, fin=fu, fa=F(40, 26),
             twin=True)
    assert k.eng.in_dtype == torch.uint8
    assert set(k.stream(stimulus(k.rng, fu, 3, 1500), [1, 701], what="unsigned")) == {"generic"}
    k = Case(16, 8, "FOLD_EVEN", fo, out_bytes, seed=34, pairs=True, force_generic=True)
    assert set(k.stream(stimulus(k.rng, FIN, 3, 1500), [1, 701], what="force_generic")) == {"generic"}
    # 80 taps per phase: a long sub-filter on int16 rows, under the flag the exact kernels (there is no byte form of the long kernels)
    k = Case(80, 4, "FOLD_ANTI", fo, out_bytes, seed=35, coeff_bits=12, twin=True)
    paths = k.stream(stimulus(k.rng, FIN, 3, 1500), [1, 701], what="80 taps")
    assert set(paths) <= set(VALU), paths                   # (never "mfma_long")


# ---- 5. confinement ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_bytes", [True, False], ids=["out1", "out2"])
@pytest.mark.parametrize("ftype,n_taps,ifac", [("FOLD_ANTI", 12, 4), ("FOLD_EVEN", 16, 4), ("FOLD_EVEN", 16, 7), ("FOLD_ANTI", 12, 5)])
def test_no_byte_outside_the_output_rows_is_written(ftype, n_taps, ifac, out_bytes):
    """sentinel rows 16 bytes into a pitch that exceeds the row by a number that is no multiple of 16, one more row behind the last; the first
    call of a folded core starts IF outputs in front of its row (out_off = -IF) and writes them nowhere"""
    fo = FO8 if out_bytes else FO16
    k = Case(n_taps, ifac, ftype, fo, out_bytes, seed=41 + ifac)
    sentinel = 0x5A if out_bytes else 0x5A5A
    lead = 16 if out_bytes else 8
    for call, n in enumerate((1056, 700)):
        x = stimulus(k.rng, FIN, 3, 1400)[:, :n]
        no = k.eng.out_count(n)
        pad = 20 + (-no) % 4                                # pitch on the dword grid, 20 .. 23 beyond the row
        buf = torch.full((4, lead + no + pad), sentinel, dtype=k.eng.out_dtype, device="cuda")
        out = buf[:3, lead:lead + no]
        y = k.eng.run(rows(x, torch.int8), out=out)
        want = k.orc.run(k.c, k.sg, k.corr, x)
        same(words(y), want, "call %d" % call)
        if call == 1 or ftype == "FOLD_ANTI" or (ifac * (1 if out_bytes else 2)) % 4 == 0:
            assert k.eng.path == "mfma_gen", (call, k.eng.path)
        b = words(buf)
        assert (b[:3, :lead] == sentinel).all(), "call %d: bytes in front of a row" % call
        assert (b[:3, lead + no:] == sentinel).all() and (b[3] == sentinel).all(), "call %d: bytes behind a row" % call


# ---- 6. stream state ---------------------------------------------------------------------------------------------------------------------------
def test_control_words_reloaded_between_calls():
    """the group emitted by the first sample of a call carries the sums formed with the OLD coefficients, combined with the NEW sign / corr"""
    x = stimulus(np.random.default_rng(51), FIN, 2, 2200)
    eng = A.PolyIntr(16, 40, 4, "FOLD_EVEN", FIN, FC, FA, FO8, n_channels=2, in_bytes=True, out_bytes=True)
    orc = OraclePolyIntr(16, 40, 4, "FOLD_EVEN", ofmt(FIN), ofmt(FC), ofmt(FA), ofmt(FO8), n_ch=2)
    paths = []
    for k, (a, b) in enumerate([(0, 700), (700, 701), (701, 1500), (1500, 2200)]):
        c = rand_fmt(np.random.default_rng(100 + k), FC, (40,))
        sign, corr = [1, 1, 1, 1], ([3, 2, 1, 0] if k != 1 else [0, 1, 2, 3])
        eng.set_ctrl(c, sign, corr)
        y = eng.run(rows(x[:, a:b], torch.int8))
        paths.append(eng.path)
        same(words(y), orc.run(c, sign, corr, x[:, a:b]), "call %d" % k)
    assert paths[0] == paths[2] == paths[3] == "mfma_gen", paths


def _pair(out_bytes_a, out_bytes_b, in_bytes_b=True, seed=61):
    rng = np.random.default_rng(seed)
    csz, c, sg, corr = control(rng, 16, 4, "FOLD_EVEN", True)
    a = A.PolyIntr(16, csz, 4, "FOLD_EVEN", FIN, FC, FA, FO8, n_channels=3, in_bytes=True, out_bytes=out_bytes_a)
    b = A.PolyIntr(16, csz, 4, "FOLD_EVEN", FIN, FC, FA, FO8, n_channels=3, in_bytes=in_bytes_b, out_bytes=out_bytes_b)
    a.set_ctrl(c, sg, corr)
    b.set_ctrl(c, sg, corr)
    orc = OraclePolyIntr(16, csz, 4, "FOLD_EVEN", ofmt(FIN), ofmt(FC), ofmt(FA), ofmt(FO8), n_ch=3)
    return rng, a, b, lambda x: orc.run(c, sg, corr, x)


@pytest.mark.parametrize("out_a,out_b", [(True, True), (True, False), (False, True)], ids=["same", "out1_to_out2", "out2_to_out1"])
def test_a_state_blob_continues_the_stream_in_a_fresh_flagged_handle(out_a, out_b):
    rng, a, b, orc = _pair(out_a, out_b)
    x = stimulus(rng, FIN, 3, 1500)
    same(words(a.run(rows(x[:, :780], torch.int8))), orc(x[:, :780]), "first handle")
    assert a.path == "mfma_gen"
    b.set_state(a.state())
    y = b.run(rows(x[:, 780:], torch.int8))
    assert b.path == "mfma_gen" and y.dtype == (torch.int8 if out_b else torch.int16)
    same(words(y), orc(x[:, 780:]), "second handle")


def test_blobs_of_flagged_and_unflagged_handles_refuse_each_other():
    rng, a, b, orc = _pair(True, False, in_bytes_b=False)
    x = stimulus(rng, FIN, 3, 700)
    a.run(rows(x, torch.int8))
    b.run(rows(x, torch.int16))
    for src, dst in ((a, b), (b, a)):
        with pytest.raises(A.AcdspError) as e:
            dst.set_state(src.state())
        assert e.value.code == 1, e.value                   # ACDSP_EINVAL
    x2 = stimulus(rng, FIN, 3, 700)                         # both handles are where they were
    want = orc(np.concatenate([x, x2], axis=1))[:, -700 * 4:]
    same(words(a.run(rows(x2, torch.int8))), want, "flagged")
    same(words(b.run(rows(x2, torch.int16))), want, "unflagged")


def test_clone_mid_stream_and_reset():
    rng, a, _, orc = _pair(True, True, seed=62)
    x = stimulus(rng, FIN, 3, 2100)
    same(words(a.run(rows(x[:, :700], torch.int8))), orc(x[:, :700]), "in front of the clone")
    twin = a.clone()
    assert twin.in_bytes and twin.out_bytes and twin.in_dtype == torch.int8 and twin.out_dtype == torch.int8
    assert A._lib.lib.acdsp_polyintr_in_elem_bytes(twin._h) == 1 and A._lib.lib.acdsp_polyintr_out_elem_bytes(twin._h) == 1
    want = orc(x[:, 700:1400])
    same(words(a.run(rows(x[:, 700:1400], torch.int8))), want, "original")
    same(words(twin.run(rows(x[:, 700:1400], torch.int8))), want, "clone")
    assert a.path == twin.path == "mfma_gen"
    torch.cuda.synchronize()
    a.reset()                                               # a new stream: the first sample emits nothing again
    _, _, _, fresh = _pair(True, True, seed=62)
    y = a.run(rows(x[:, 1400:], torch.int8))
    assert y.shape[1] == 699 * 4
    same(words(y), fresh(x[:, 1400:]), "behind reset")


# ---- 7. chaining -------------------------------------------------------------------------------------------------------------------------------
def test_a_byte_interpolator_feeds_a_byte_fir_and_is_fed_by_one():
    rng = np.random.default_rng(71)
    n_ch, n, n_taps = 3, 1056, 31
    csz, c, sg, corr = control(rng, 16, 4, "FOLD_EVEN", True)
    h = rng.integers(-2000, 2001, size=n_taps, dtype=np.int64)
    ffa, ffo16, ffo8 = F(48, 28), F(16, 6, True, "RND", "SAT"), F(8, 2, True, "RND", "SAT")
    x = stimulus(rng, FIN, n_ch, 2 * n)
    # interpolator -> FIR: the FIR's IN_TYPE is the interpolator's OUT_TYPE, its input tensor the interpolator's output tensor
    intr = A.PolyIntr(16, csz, 4, "FOLD_EVEN", FIN, FC, FA, FO8, n_channels=n_ch, in_bytes=True, out_bytes=True)
    intr.set_ctrl(c, sg, corr)
    fir = A.Fir(n_taps, "SHIFT_REG", F(8, 2), FC, ffa, ffo16, n_channels=n_ch, kind="load", in_bytes=True)
    fir.set_coeffs(h)
    o_i = OraclePolyIntr(16, csz, 4, "FOLD_EVEN", ofmt(FIN), ofmt(FC), ofmt(FA), ofmt(FO8), n_ch=n_ch)
    o_f = OracleFir(n_taps, "SHIFT_REG", ofmt(F(8, 2)), ofmt(FC), ofmt(ffa), ofmt(ffo16), n_ch=n_ch)
    for a in (0, n):
        y1 = intr.run(rows(x[:, a:a + n], torch.int8))
        assert y1.dtype == torch.int8 == fir.in_dtype
        y2 = fir.run(y1)
        m = o_i.run(c, sg, corr, x[:, a:a + n])
        same(words(y1), m, "interpolator")
        same(words(y2)[:, :m.shape[1]], o_f.run(h, m), "FIR behind it")
    assert intr.path == "mfma_gen"
    # FIR -> interpolator
    fir = A.Fir(n_taps, "SHIFT_REG", F(8, 2), FC, ffa, ffo8, n_channels=n_ch, kind="load", in_bytes=True, out_bytes=True)
    fir.set_coeffs(h)
    intr = A.PolyIntr(16, csz, 4, "FOLD_EVEN", FIN, FC, FA, FO16, n_channels=n_ch, in_bytes=True)
    intr.set_ctrl(c, sg, corr)
    o_f = OracleFir(n_taps, "SHIFT_REG", ofmt(F(8, 2)), ofmt(FC), ofmt(ffa), ofmt(ffo8), n_ch=n_ch)
    o_i = OraclePolyIntr(16, csz, 4, "FOLD_EVEN", ofmt(FIN), ofmt(FC), ofmt(FA), ofmt(FO16), n_ch=n_ch)
    for a in (0, n):
        y1 = fir.run(rows(x[:, a:a + n], torch.int8))
        assert y1.dtype == torch.int8 == intr.in_dtype
        y2 = intr.run(y1)
        m = o_f.run(h, x[:, a:a + n])
        same(words(y1), m, "FIR")
        same(words(y2), o_i.run(c, sg, corr, m), "interpolator behind it")
    assert intr.path == "mfma_gen"


# ---- 8. graph capture --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_bytes", [True, False], ids=["out1", "out2"])
def test_a_captured_pair_of_calls_replays_like_eager_calls_on_a_twin(out_bytes):
    """calls on the matrix-core path with their side-stream fork and join, captured behind the stream's first call and replayed twice on changed
    input contents.  The family flips its history and saved sums between two buffers on every call, so -- as on int16 rows (INTEGRATION.md,
    "captured in pairs") -- a graph holds an even number of calls: two here, and the two replays continue the stream as four eager calls do"""
    k = Case(16, 8, "FOLD_EVEN", FO8 if out_bytes else FO16, out_bytes, seed=81, pairs=True)
    twin = k.eng.clone()
    n = 1056
    side = torch.cuda.Stream()
    x0 = stimulus(k.rng, FIN, 3, n)
    xd = rows(x0, torch.int8)
    with torch.cuda.stream(side):
        y = k.eng.run(xd, out=out_rows(k.eng, n))
    side.synchronize()
    xds = [xd, rows(x0, torch.int8)]                        # (behind the stream's first call: IF outputs per input sample from here on)
    outs = [out_rows(k.eng, n), out_rows(k.eng, n)]
    want = k.orc.run(k.c, k.sg, k.corr, x0)
    same(words(y), want, "eager call in front")
    same(words(twin.run(rows(x0, torch.int8))), want, "twin, first call")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for xd_, out in zip(xds, outs):
            k.eng.run(xd_, out=out)
            assert k.eng.path == "mfma_gen"
    torch.cuda.synchronize()
    for r in range(2):
        xs = [stimulus(np.random.default_rng(800 + 2 * r + i), FIN, 3, n) for i in range(2)]
        for xd_, x, out in zip(xds, xs, outs):
            xd_.copy_(torch.from_numpy(x).to(torch.int8))
            out.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for i, (x, out) in enumerate(zip(xs, outs)):
            want = k.orc.run(k.c, k.sg, k.corr, x)
            same(words(out), want, "replay %d, call %d" % (r, i))
            same(words(twin.run(rows(x, torch.int8))), want, "twin, eager call %d" % (2 * r + i))
            assert twin.path == "mfma_gen"


# ---- 9. the other entry points -----------------------------------------------------------------------------------------------------------------
def test_node_with_three_shards_on_device_0():
    rng = np.random.default_rng(91)
    n_ch, n = 5, 1056
    csz, c, sg, corr = control(rng, 16, 4, "FOLD_EVEN", True)
    node = A.NodePolyIntr(16, csz, 4, "FOLD_EVEN", FIN, FC, FA, FO8, n_ch, [0, 0, 0], in_bytes=True, out_bytes=True)
    node.set_ctrl(c, sg, corr)
    assert node.in_dtype == torch.int8 and node.out_dtype == torch.int8
    orc = OraclePolyIntr(16, csz, 4, "FOLD_EVEN", ofmt(FIN), ofmt(FC), ofmt(FA), ofmt(FO8), n_ch=n_ch)
    x = stimulus(rng, FIN, n_ch, 2 * n)
    for a in (0, n):
        xs = node.alloc(FIN, n, as_bytes=True)             # (one block per shard, all of one row pitch)
        for t, (lo, hi) in zip(xs, node.slices):
            t.copy_(torch.from_numpy(np.ascontiguousarray(x[lo:hi, a:a + n])).to(torch.int8))
        ys = node.run(xs)
        assert all(y.dtype == torch.int8 for y in ys)
        same(np.concatenate([words(y) for y in ys]), orc.run(c, sg, corr, x[:, a:a + n]), "call at %d" % a)
    assert all(A.PATHS[A._lib.lib.acdsp_polyintr_path(node.shard_handle(s))] == "mfma_gen" for s in range(node.n_shards))


@pytest.mark.parametrize("fin,fo,fa", [(FIN, FO8, FA), (F(8, 8, False), F(8, 8, False, "RND", "SAT"), F(40, 26))], ids=["int8", "uint8"])
def test_run_host_on_numpy_byte_rows(fin, fo, fa):
    rng = np.random.default_rng(92)
    csz, c, sg, corr = control(rng, 12, 4, "FOLD_ANTI", False)
    x = stimulus(rng, fin, 3, 1400)
    for ob in (True, False):
        fo_ = fo if ob else F(16, fo.I + (0 if fo.S else 1), True, "RND", "SAT")   # (int16 rows: a signed type, read back as int16)
        host = A.PolyIntr(12, csz, 4, "FOLD_ANTI", fin, FC, fa, fo_, n_channels=3, in_bytes=True, out_bytes=ob)
        dev = A.PolyIntr(12, csz, 4, "FOLD_ANTI", fin, FC, fa, fo_, n_channels=3, in_bytes=True, out_bytes=ob)
        orc = OraclePolyIntr(12, csz, 4, "FOLD_ANTI", ofmt(fin), ofmt(FC), ofmt(fa), ofmt(fo_), n_ch=3)
        host.set_ctrl(c, sg, corr)
        dev.set_ctrl(c, sg, corr)
        for a, b in ((0, 700), (700, 1400)):
            y = host.run_host(x[:, a:b].astype(np_bytes(fin)))
            assert y.dtype == (np_bytes(fo_) if ob else np.int16)
            same(y.astype(np.int64), words(dev.run(rows(x[:, a:b], dev.in_dtype))), "run_host against run, out_bytes %s" % ob)
            same(y.astype(np.int64), orc.run(c, sg, corr, x[:, a:b]), "run_host against the oracle, out_bytes %s" % ob)
