"""Child process of tests/test_knobs_gpu.py (a plain script: pytest does not collect it).

    python tests/knob_child.py BATTERY [BATTERY ...]
    python tests/knob_child.py --oracle-only [BATTERY ...]     (no GPU: stimulus and oracle halves only, with their CPU time)

libacdsp.so reads its ACDSP_* switches once per process, so each switch setting needs a process of its own.  This script never sets one: the
parent does.  It runs the named batteries on cuda:0, compares every output word with the CPU oracle (the pairings of tests/test_fuzz_gpu.py;
nothing is compared with another leg's GPU output) and prints one JSON line per battery:

    {"battery": ..., "cases": n, "mismatches": n, "first": "..." or null, "witness": {"case.field": value}, "state_size": {"case": bytes}}

witness: what the ABI reports about the kernel that ran (path, kernel class, mfma_epilogue(), mfma_issued(), the path properties).
Exit status 0 only when every battery ran and no word differed.

Every FIR / CIC / poly stream runs as three calls -- one long, one shorter than the history, one long -- so that both history buffers and the
carry are exercised; the FIR batteries use 9 channels (one partial group of 8)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

ORACLE_ONLY = "--oracle-only" in sys.argv[1:]
if "--help" in sys.argv[1:] or "-h" in sys.argv[1:]:
    print(__doc__)
    sys.exit(0)
if ORACLE_ONLY:
    os.environ.setdefault("ACDSP_NO_TORCH_INIT", "1")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ac_dsp_amd as A  # noqa: E402
from oracle import OracleFir, OracleCic, OraclePolyDec, OraclePolyIntr, OracleIntgDump, OracleMvAvg  # noqa: E402
from helpers import ofmt, windowed_sinc  # noqa: E402
from test_fuzz_gpu import FIR_TYPES, FIR_OUTS, rand_raw, padded_view  # noqa: E402

GPU = not ORACLE_ONLY
F = A.Fmt
OUT16 = FIR_OUTS[0]                                  # <16,2,RND,SAT>
T16 = FIR_TYPES[0]                                   # <16,2> x <16,2> into <40,12>


class Result:
    def __init__(self, battery):
        self.battery, self.cases, self.mismatches, self.first, self.witness, self.state_size = battery, 0, 0, None, {}, {}

    def compare(self, case, call, y, yo):
        if not GPU:
            return
        y = np.asarray(y).astype(np.int64)
        if y.shape != yo.shape:
            self.mismatches += 1
            self.first = self.first or "%s call %d: shape %s, oracle %s" % (case, call, y.shape, yo.shape)
            return
        bad = np.argwhere(y != yo)
        if bad.size:
            self.mismatches += len(bad)
            self.first = self.first or "%s call %d: %d words differ, first at %s: got %d want %d" % (case, call, len(bad), bad[0].tolist(), y[tuple(bad[0])], yo[tuple(bad[0])])

    def line(self):
        return json.dumps(dict(battery=self.battery, cases=self.cases, mismatches=self.mismatches, first=self.first, witness=self.witness, state_size=self.state_size))


def dev(x, fmt):
    return torch.from_numpy(np.ascontiguousarray(x)).to(A.torch_dtype_for(fmt)).cuda()


def host(y):
    return y.cpu().numpy().astype(np.int64)


def fir_witness(R, case, fir):
    e = fir.mfma_epilogue()
    R.witness[case + ".path"], R.witness[case + ".kernel"], R.witness[case + ".issued"] = fir.path, fir.kernel, fir.mfma_issued()
    if e is not None:
        R.witness[case + ".epi"], R.witness[case + ".cshift"], R.witness[case + ".flip"] = e[0], e[1], e[2]
    R.state_size[case] = A.lib.acdsp_fir_state_size(fir._h)


def fir_case(R, case, n_taps, ftype, fin, fc, fa, fo, coeffs, lens, n_ch=9, kind="load", seed=0, edit=None):
    """coeffs: one set, or a list with the set to load in front of each call (None: keep the last one)"""
    R.cases += 1
    rng = np.random.default_rng(seed)
    sets = coeffs if isinstance(coeffs, list) else [coeffs] + [None] * (len(lens) - 1)
    x = rand_raw(rng, fin, (n_ch, sum(lens)))
    if edit:
        edit(x)
    orc = OracleFir(n_taps, ftype, ofmt(fin), ofmt(fc), ofmt(fa), ofmt(fo), n_ch=n_ch)
    fir = A.Fir(n_taps, ftype, fin, fc, fa, fo, n_channels=n_ch, kind=kind) if GPU else None
    a, c = 0, None
    for i, n in enumerate(lens):
        if sets[i] is not None:
            c = sets[i]
            if GPU:
                fir.set_coeffs(c)
        yo = orc.run(c, x[:, a:a + n])
        if GPU:
            R.compare(case, i, host(fir.run(dev(x[:, a:a + n], fin))), yo)
            if i == 0:
                fir_witness(R, case, fir)
        a += n
    return fir


def lossless_acc(fin, fc, guard):
    return F(fin.W + fc.W + guard, fin.I + fc.I + guard)


# ------------------------------------------------------------------------------------------------ FIR on the int8 matrix-core kernels
LONG_BIG = (8192 + 40, 17, 3000)      # more than 9 K-blocks: whole 2048-sample double steps for fir_mfma_big2_kernel, then the single-wide kernel
LONG = (4096 + 77, 17, 2500)


def bat_fir_mid(R):
    fir_case(R, "t319", 319, "SHIFT_REG", T16[0], T16[1], T16[2], OUT16, windowed_sinc(319, 0.05, T16[1]), LONG_BIG, seed=1)
    # at unit gain the set's high-byte band is exactly the 5 K-blocks of the compiled shape: both kernels issue the same count.  Gain 0.3 leaves
    # 3 blocks: the register-resident shape still issues 5, the LDS-resident kernel 3 -- the witness
    fir_case(R, "t319_g03", 319, "SHIFT_REG", T16[0], T16[1], T16[2], OUT16, windowed_sinc(319, 0.05, T16[1], gain=0.3), LONG_BIG, seed=101)


def bat_fir_reg33(R):
    fir_case(R, "t1025", 1025, "SHIFT_REG", T16[0], T16[1], T16[2], OUT16, windowed_sinc(1025, 0.05, T16[1]), LONG_BIG, seed=2)
    fir_case(R, "t1025_g03", 1025, "SHIFT_REG", T16[0], T16[1], T16[2], OUT16, windowed_sinc(1025, 0.05, T16[1], gain=0.3), LONG_BIG, seed=102)   # (see fir_mid)


def bat_fir_epi4(R):
    rng = np.random.default_rng(3)
    c = np.minimum(rand_raw(rng, T16[1], (300,)), 32639)
    fir_case(R, "dense300", 300, "SHIFT_REG", T16[0], T16[1], T16[2], OUT16, c, LONG_BIG, seed=3)
    # uniform taps average |digit| = 64 in both byte planes: at 300 taps 2^8 mid + ll still fits int32 (the 32-bit class, on either side of the switch;
    # it passes int32 from about 511 taps on).  Both digits of every tap at 112 .. 127, random signs: 128 * 256 * sum(|hi| + |lo|) > 2^31 -- EPI 4
    dig = rng.integers(112, 128, size=(2, 300))
    fs = rng.choice([-1, 1], size=300) * (256 * dig[0] + dig[1])
    assert np.abs(fs).max() <= 32639 and 128 * 256 * int(dig.sum()) > 1 << 31
    fir_case(R, "full_scale300", 300, "SHIFT_REG", T16[0], T16[1], T16[2], OUT16, fs.astype(np.int64), LONG_BIG, seed=103)


def bat_fir_gq(R):
    c = np.random.default_rng(4).integers(-20000, 20000, size=255, dtype=np.int64)
    fir_case(R, "rnd_zero_sat_zero", 255, "SHIFT_REG", T16[0], T16[1], T16[2], FIR_OUTS[7], c, LONG, seed=4)
    fir_case(R, "trn_zero_sat_sym", 255, "SHIFT_REG", T16[0], T16[1], T16[2], FIR_OUTS[8], c, LONG, seed=5)


def bat_fir_nar(R):
    raw = rand_raw(np.random.default_rng(6), T16[1], (255,))
    # <12,5,RND_CONV,SAT_SYM>: narrow AND a general rounding mode -- the generic epilogue on either side of the switch (no NAR instantiation)
    fir_case(R, "w12_conv_sym", 255, "SHIFT_REG", T16[0], T16[1], T16[2], FIR_OUTS[6], raw // 8, LONG, seed=6)
    # the NAR instantiations skip high-plane blocks only where the set leaves them empty: |c| < 128 (raw // 256), narrow OUT and general mode
    fir_case(R, "w12_empty_hi", 255, "SHIFT_REG", T16[0], T16[1], T16[2], F(12, 5, True, "RND", "SAT"), raw // 256, LONG, seed=7)
    fir_case(R, "gq_empty_hi", 255, "SHIFT_REG", T16[0], T16[1], T16[2], FIR_OUTS[7], raw // 256, LONG, seed=8)


def bat_fir_cshift(R):
    fin, fc = F(14, 4), F(12, 2)
    c = rand_raw(np.random.default_rng(9), fc, (63,))
    # every product bit kept in a 16-bit OUT_TYPE (F_out = F_in + F_coeff = 20): nothing left to shift by, pre-scaled by one bit
    # (coefficients // 8: the pre-scaled high plane has to stay inside the 32-bit epilogue's bounds)
    fir_case(R, "w14_keep_all", 63, "SHIFT_REG", fin, fc, lossless_acc(fin, fc, 6), F(16, -4, True, "RND", "SAT"), c // 8, LONG, seed=9)
    # tests/test_fir_gpu.py: <8,1> end to end, 7 dropped bits against the 8 of the packed finish
    f8 = F(8, 1)
    fir_case(R, "w8", 63, "SHIFT_REG", f8, f8, F(30, 15), F(8, 1, True, "RND", "SAT"), rand_raw(np.random.default_rng(10), f8, (63,)), LONG, seed=10)


def bat_fir_u16(R):
    fin, fc = F(16, 2, False), F(16, 2)
    c = np.minimum(rand_raw(np.random.default_rng(11), fc, (100,)), 32639)
    fir_case(R, "acc44", 100, "SHIFT_REG", fin, fc, F(44, 16), OUT16, c, LONG, seed=11)
    fir_case(R, "acc34", 100, "SHIFT_REG", fin, fc, F(34, 6), OUT16, c, LONG, seed=12)       # an accumulator that may wrap


def bat_fir_rt(R):
    # TRANSPOSED, loadable: a reload between the calls, and a second one fewer than n_taps - 1 = 39 samples later
    fin, fc, fa = F(16, 2), F(16, 2), F(42, 14)
    rng = np.random.default_rng(13)
    sets = [np.minimum(rand_raw(rng, fc, (40,)), 32639) for _ in range(3)]
    fir_case(R, "reload40", 40, "TRANSPOSED", fin, fc, fa, OUT16, [sets[0], sets[1], sets[2], None], (4096 + 77, 17, 2500, 1100), seed=13)


def bat_fir_lossy(R):
    long_l = (4096 + 100, 17, 4096 + 2500)          # whole 4096-output chunks on the matrix cores, the ragged rest on the exact-order kernel
    for case, (fin, fc, fa), seed in (("w16", FIR_TYPES[15], 14), ("w28", FIR_TYPES[11], 15), ("sat20", FIR_TYPES[4], 16)):
        c = rand_raw(np.random.default_rng(seed), fc, (63,))
        if fc.W > 22:
            c = c >> (fc.W - 22)                      # three balanced base-256 digits (tests/test_fuzz_gpu.py)
        fo = OUT16 if fin.W <= 16 else FIR_OUTS[4]    # (the class-B ring shapes of 4-byte samples write 4- or 8-byte outputs)
        fir_case(R, case, 63, "SHIFT_REG", fin, fc, fa, fo, c, long_l, seed=seed)


def bat_fir_unaligned(R):
    # rows start 3 elements into a wider buffer; stride n + 3 + tail odd; the output rows start one element in
    c = np.random.default_rng(17).integers(-20000, 20000, size=255, dtype=np.int64)
    R.cases += 1
    rng = np.random.default_rng(17)
    fin, fc, fa = T16
    n_ch, lens = 9, LONG
    x = rand_raw(rng, fin, (n_ch, sum(lens)))
    orc = OracleFir(255, "SHIFT_REG", ofmt(fin), ofmt(fc), ofmt(fa), ofmt(OUT16), n_ch=n_ch)
    fir = None
    if GPU:
        fir = A.Fir(255, "SHIFT_REG", fin, fc, fa, OUT16, n_channels=n_ch)
        fir.set_coeffs(c)
    a = 0
    for i, n in enumerate(lens):
        yo = orc.run(c, x[:, a:a + n])
        if GPU:
            tail = 8 + (n + 3 + 8 + 1) % 2               # readable up to the next multiple of 8 samples, odd stride
            xv = padded_view(x[:, a:a + n], torch.int16, 3, tail)
            assert xv.stride(0) % 2 == 1 and xv.data_ptr() % 16 != 0
            out = torch.zeros((n_ch, n + 1 + 8 + n % 2), dtype=torch.int16, device="cuda")[:, 1:]
            assert out.stride(0) % 2 == 1
            R.compare("lead3", i, host(fir.run(xv, out)[:, :n]), yo)
            if i == 0:
                fir_witness(R, "lead3", fir)
        a += n


# ------------------------------------------------------------------------------------------------ saturation-free saturating accumulators
def full_scale(fmt, shape, rng):
    """tests/test_satfree_bounds_gpu.py: rows all max, all min, alternating, random"""
    lo, hi = (-(1 << (fmt.W - 1)), (1 << (fmt.W - 1)) - 1) if fmt.S else (0, (1 << fmt.W) - 1)
    x = rng.integers(lo, hi + 1, size=shape, dtype=np.int64)
    x[0], x[1] = hi, lo
    x[2, ::2], x[2, 1::2] = hi, lo
    return x


def fill_greedy(n, total):
    c = np.zeros(n, dtype=np.int64)
    for i in range(n):
        c[i] = min(total, 32767)
        total -= c[i]
    assert total == 0
    return c


def bat_satfree(R):
    # FIR (tests/test_fir_gpu.py): sum|c| = 32737, 32737 * 2^15 < 2^30 - 1 -- one step inside the bound of ACC <31,3,TRN,SAT>
    def edge(x):
        x[0, :] = -32768
        x[1, ::2] = 32767
    fir_case(R, "fir", 32, "SHIFT_REG", F(16, 2), F(16, 2), F(31, 3, True, "TRN", "SAT"), F(16, 3, True, "RND", "SAT"),
             np.array([1023] * 31 + [1024], dtype=np.int64), (4096 + 77, 17, 2500), seed=18, edit=edge)
    # ac_poly_dec: sum|c| = 65535 < 2^16 into ACC <32,4,TRN,SAT>
    R.cases += 1
    nt, df, n_ch = 8, 4, 4
    fin, fc, fa, fo = F(16, 2), F(16, 2), F(32, 4, True, "TRN", "SAT"), F(32, 4)
    c = fill_greedy(nt * df, 65535)
    orc = OraclePolyDec(nt, df, ofmt(fin), ofmt(fc), ofmt(fa), ofmt(fo), n_ch=n_ch)
    eng = None
    if GPU:
        eng = A.PolyDec(nt, df, fin, fc, fa, fo, n_channels=n_ch)
        eng.set_coeffs(c)
    rng = np.random.default_rng(65535)
    for i, groups in enumerate((64 * 4, 3, 700)):
        x = full_scale(fin, (n_ch, groups * df), rng)
        yo = orc.run(c, x)
        if GPU:
            R.compare("polydec", i, host(eng.run(dev(x, fin))), yo)
            if i == 0:
                R.witness["polydec.path"] = eng.path
    # ac_intg_dump: 64 rounds of <16,8> into ACC <23,15,TRN,SAT>: 64 * 2^15 = 2^21 <= 2^22 - 1 (at 22 bits the same blocks could saturate)
    R.cases += 1
    ns, chn, n_obj, rounds = 256, 4, 4, 64
    fin, fa, fo = F(16, 8), F(23, 15, True, "TRN", "SAT"), F(32, 24)
    orc = OracleIntgDump(ns, chn, ofmt(fin), ofmt(fa), ofmt(fo), n_obj=n_obj)
    eng = A.IntgDump(ns, chn, fin, fa, fo, n_objects=n_obj) if GPU else None
    rng = np.random.default_rng(6423)
    for i, nb in enumerate((64, 8)):
        n_sample = [rounds] * nb
        x = full_scale(fin, (n_obj, rounds * chn * nb), rng)
        yo = orc.run(x, n_sample)
        if GPU:
            R.compare("intg", i, host(eng.run(dev(x, fin), n_sample)), yo)
            if i == 0:
                R.witness["intg.path"] = eng.path
    # ac_mv_avg: sum|c| = 262138 at the bound 2 sum|c| + TAPS + 1 <= 2^19 - 1 of ACC <20,12,TRN,SAT>
    R.cases += 1
    taps, n_sample, n_frames = 9, 1024, 4
    fin, fc, fa, fo = F(16, 8), F(16, 2), F(20, 12, True, "TRN", "SAT"), F(20, 12)
    c = fill_greedy(taps, 262138)
    x = full_scale(fin, (4, n_sample * n_frames), np.random.default_rng(262138))
    yo = OracleMvAvg(taps, "MIRROR", ofmt(fin), ofmt(fc), ofmt(fa), ofmt(fo), n_obj=4).run(c, x, n_sample)
    if GPU:
        eng = A.MvAvg(4096, taps, "MIRROR", fin, fc, fa, fo, n_objects=4)
        eng.set_coeffs(c)
        R.compare("mvavg", 0, host(eng.run(dev(x, fin), n_sample)), yo)
        R.witness["mvavg.path"] = eng.path


# ------------------------------------------------------------------------------------------------ the multi-plane kernels (fir_gen.hip) and CIC
def bat_fir_gen(R):
    fin, fc, fa = FIR_TYPES[2]                                        # <36,21> x <16,1> into <60,30>
    c = rand_raw(np.random.default_rng(19), fc, (100,))
    fir_case(R, "w36", 100, "SHIFT_REG", fin, fc, fa, FIR_OUTS[4], c, LONG, seed=19)


def cic_case(R, case, interp, Rr, M, N, fin, n_ch, lens, seed):
    R.cases += 1
    rng = np.random.default_rng(seed)
    it = Fmt_of_cic(interp, Rr, M, N, fin)
    fout = F(it.W, it.I)
    orc = OracleCic(interp, Rr, M, N, ofmt(fin), ofmt(fout), n_ch=n_ch)
    cic = A.Cic(interp, Rr, M, N, fin, fout, n_channels=n_ch) if GPU else None
    for i, n in enumerate(lens):
        x = rand_raw(rng, fin, (n_ch, n))
        yo = orc.run(x)
        if GPU:
            xv = padded_view(x, A.torch_dtype_for(fin), 0, (-n) % 16)      # whole 16-sample slots, 16-byte row strides: what the matrix-core kernels take
            R.compare(case, i, host(cic.run(xv)), yo)
            if i == 0 or (interp and n >= 1024):                     # (the interpolator reports the path of the last run())
                R.witness[case + ".path"] = cic.path
            R.state_size[case] = A.lib.acdsp_cic_state_size(cic._h)


def Fmt_of_cic(interp, Rr, M, N, fin):
    it = A.Fmt()
    d = A.CicDesc(int(bool(interp)), Rr, M, N, 1, fin, fin, 0, 0)
    A._lib.check(A.lib.acdsp_cic_int_type(d, it))
    return it


def bat_cic_gen(R):
    cic_case(R, "r8n5", False, 8, 1, 5, F(32, 16), 3, (8 * 1000, 17, 8 * 700 + 3), 20)


def bat_cic_dec(R):
    # the decimation phase is not 0 at the start of the second and third call (17 and 17 + 16 R 256 inputs in)
    for Rr, M, N in ((64, 2, 3), (16, 1, 4)):
        for n_ch in (3, 65):
            cic_case(R, "r%d_c%d" % (Rr, n_ch), False, Rr, M, N, F(16, 1), n_ch, (16 * Rr * 256, 17, 1000), 21 + n_ch)


def bat_cic_up(R):
    cic_case(R, "r8n5", True, 8, 1, 5, F(16, 8), 3, (1, 300, 2500), 22)


def bat_polydec(R):
    R.cases += 1
    nt, df, n_ch = 8, 5, 9
    fin, fc = F(16, 2), F(16, 2)
    fa, fo = lossless_acc(fin, fc, 9), OUT16
    rng = np.random.default_rng(23)
    c = rand_raw(rng, fc, (nt * df,))
    orc = OraclePolyDec(nt, df, ofmt(fin), ofmt(fc), ofmt(fa), ofmt(fo), n_ch=n_ch)
    eng = None
    if GPU:
        eng = A.PolyDec(nt, df, fin, fc, fa, fo, n_channels=n_ch)
        eng.set_coeffs(c)
    for i, groups in enumerate((2048 + 16, 3, 704)):
        x = rand_raw(rng, fin, (n_ch, groups * df))
        yo = orc.run(c, x)
        if GPU:
            R.compare("nt8df5", i, host(eng.run(dev(x, fin))), yo)
            if i == 0:
                R.witness["nt8df5.path"] = eng.path


def bat_polyintr(R):
    R.cases += 1
    n_taps, ifac, n_ch = 15, 3, 9
    csz = (n_taps - 1) // 2 + (n_taps // 2 + 1) * (ifac - 1) + 1        # FOLD_ODD (tests/test_fuzz_gpu.py)
    fin, fc = F(16, 2), F(16, 2)
    fa, fo = lossless_acc(fin, fc, 9), OUT16
    rng = np.random.default_rng(24)
    # the matrix-core class (tests/test_polyintr_gpu.py: check_up): every sign[j] set, so that the folded cores stay linear in the samples
    ci, sign, corr = rng.integers(-4096, 4096, size=csz, dtype=np.int64), np.ones(ifac, dtype=np.int64), ifac - 1 - np.arange(ifac)
    orc = OraclePolyIntr(n_taps, csz, ifac, "FOLD_ODD", ofmt(fin), ofmt(fc), ofmt(fa), ofmt(fo), n_ch=n_ch)
    eng = None
    if GPU:
        eng = A.PolyIntr(n_taps, csz, ifac, "FOLD_ODD", fin, fc, fa, fo, n_channels=n_ch)
        eng.set_ctrl(ci, sign, corr)
    for i, n in enumerate((1, 37, 1500)):
        x = rand_raw(rng, fin, (n_ch, n))
        yo = orc.run(ci, sign, corr, x)
        if GPU:
            R.compare("fold_odd15", i, host(eng.run(padded_view(x, torch.int16, 0, (-n) % 16))), yo)   # 16-byte row strides
            R.witness["fold_odd15.path"] = eng.path                     # of the last (long) call


def ddc_case(R, case, n_ch, n_total, cut, seed):
    from test_ddc_gpu import CFG5, oracle_cascade
    R.cases += 1
    g, fo = CFG5, F(24, 9, True, "RND", "SAT")
    rng = np.random.default_rng(seed)
    x = rand_raw(rng, g["cin"], (n_ch, n_total))
    c = windowed_sinc(g["n_taps"], 0.2, g["fc"])
    mid = Fmt_of_cic(False, g["R"], g["M"], g["N"], g["cin"])
    yo = oracle_cascade(g["R"], g["M"], g["N"], g["cin"], F(mid.W, mid.I), g["n_taps"], "SHIFT_REG", g["fc"], g["fa"], fo, c, x, [cut])
    if GPU:
        ddc = A.Ddc(g["R"], g["M"], g["N"], g["cin"], g["n_taps"], "SHIFT_REG", g["fc"], g["fa"], fo, n_channels=n_ch)
        ddc.set_coeffs(c)
        ys = []
        for a, b in ((0, cut), (cut, n_total)):
            big = torch.zeros((n_ch, (b - a + 15) // 16 * 16), dtype=torch.int16, device="cuda")   # whole 16-sample slots readable
            big[:, :b - a] = dev(x[:, a:b], g["cin"])
            ys.append(host(ddc.run(big[:, :b - a])))
        R.compare(case, 0, np.concatenate(ys, axis=1), yo)
        R.witness[case + ".path"] = ddc.path
        R.state_size[case] = A.lib.acdsp_ddc_state_size(ddc._h)


def bat_ddc(R):
    ddc_case(R, "cfg5", 2, 16 * 3000, 16 * 1000 + 5, 25)


# ------------------------------------------------------------------------------------------------ ac_intg_dump, ac_mv_avg
def bat_intg(R):
    ns, n_obj = 64, 5
    fin, fa = F(16, 8), F(40, 20)
    for chn in (3, 8, 4):                             # 3: matrix-core de-interleave; 8: per-load streaming kernel; 4: batched reduce-scatter kernel
        R.cases += 1
        rng = np.random.default_rng(26 + chn)
        orc = OracleIntgDump(ns, chn, ofmt(fin), ofmt(fa), ofmt(fa), n_obj=n_obj)
        eng = A.IntgDump(ns, chn, fin, fa, fa, n_objects=n_obj) if GPU else None
        for i, nb in enumerate((40, 24)):
            n_sample = [ns] * nb                      # every block dumps after NS rounds
            x = rand_raw(rng, fin, (n_obj, ns * chn * nb))
            yo = orc.run(x, n_sample)
            if GPU:
                R.compare("chn%d" % chn, i, host(eng.run(dev(x, fin), n_sample)), yo)
                R.witness["chn%d.path" % chn] = eng.path


def mv_case(R, case, taps, mode, n_sample, n_frames, fin, fa, fo, seed, out_lead=0, n_obj=3):
    R.cases += 1
    rng = np.random.default_rng(seed)
    fc = F(16, 2)
    c = rand_raw(rng, fc, (taps,))
    c = c // int((np.abs(c).sum() >> 14) + 1)         # the int32 class of the streaming kernel: sum|c| <= 32767
    x = rand_raw(rng, fin, (n_obj, n_sample * n_frames))
    yo = OracleMvAvg(taps, mode, ofmt(fin), ofmt(fc), ofmt(fa), ofmt(fo), n_obj=n_obj).run(c, x, n_sample)
    if GPU:
        eng = A.MvAvg(4096, taps, mode, fin, fc, fa, fo, n_objects=n_obj)
        eng.set_coeffs(c)
        out = None
        if out_lead:
            out = torch.zeros((n_obj, yo.shape[1] + out_lead + 5), dtype=A.torch_dtype_for(fo), device="cuda")[:, out_lead:]
        R.compare(case, 0, host(eng.run(dev(x, fin), n_sample, out)), yo)
        R.witness[case + ".path"] = eng.path


def bat_mvavg(R):
    s16, acc, o16, o32 = F(16, 8), F(40, 18), F(16, 8, True, "RND", "SAT"), F(32, 12)
    mv_case(R, "pack128", 9, "MIRROR", 128, 8, s16, acc, o16, 30)              # four frames per tile; packed 16-bit AC_SAT epilogue
    mv_case(R, "clip9_row", 9, "CLIP", 1000, 3, s16, acc, o32, 31)              # the tiles walk the row across the frame edges
    mv_case(R, "win9_row", 9, "WIN", 1000, 3, s16, acc, o16, 32)                # ... the output row (AC_WIN)
    mv_case(R, "mirror33", 33, "MIRROR", 1024, 2, s16, acc, o32, 33)            # matrix cores
    mv_case(R, "win33_run", 33, "WIN", 1024, 2, s16, acc, o16, 34, out_lead=3)  # output frames off the 16-byte boundary: aligned runs through the LDS image
    mv_case(R, "clip9_run", 9, "CLIP", 1024, 2, s16, acc, o32, 35, out_lead=3)
    mv_case(R, "mirror9_pk16", 9, "MIRROR", 1024, 2, s16, acc, o16, 36)
    mv_case(R, "w32", 9, "MIRROR", 1024, 2, F(32, 16), F(60, 30), F(32, 16, True, "RND", "SAT"), 37)


# ------------------------------------------------------------------------------------------------ host-side calls, XCD remap
def bat_host(R):
    """Fir.run_host: 27 taps x 1 sample, many calls in a row, then 27 x 64"""
    R.cases += 1
    fin, fc, fa = T16
    rng = np.random.default_rng(38)
    c = rand_raw(rng, fc, (27,)) // 2
    orc = OracleFir(27, "SHIFT_REG", ofmt(fin), ofmt(fc), ofmt(fa), ofmt(OUT16), n_ch=1)
    fir = None
    if GPU:
        fir = A.Fir(27, "SHIFT_REG", fin, fc, fa, OUT16, n_channels=1, kind="prog")
        fir.set_coeffs(c)
    for i, n in enumerate([1] * 60 + [64] * 12 + [1] * 5):
        x = rand_raw(rng, fin, (1, n))
        yo = orc.run(c, x)
        if GPU:
            R.compare("prog27", i, fir.run_host(x), yo)
    if GPU:
        fir_witness(R, "prog27", fir)


def bat_xcd(R):
    """One case per kernel family that has the XCD block remap; 8 channels / objects and lengths that give a multiple of 8 workgroups (the remap is
    off otherwise): fir_gen ring (CIC R 8 on int32: on by default; ac_poly_dec), two-stage CIC, fused cascade, ac_mv_avg streaming kernel."""
    cic_case(R, "cic_r8n5", False, 8, 1, 5, F(32, 16), 8, (8 * 512 * 4, 17, 8 * 512 * 2 + 40), 40)
    cic_case(R, "cic2_r64", False, 64, 2, 3, F(16, 1), 8, (16 * 64 * 256, 17, 1000), 41)
    ddc_case(R, "ddc_cfg5", 8, 16 * 256 * 8 * 2 + 16 * 100, 16 * 256 * 8, 42)
    mv_case(R, "mvavg", 9, "MIRROR", 1024, 4, F(16, 8), F(40, 18), F(16, 8, True, "RND", "SAT"), 43, n_obj=8)
    R.cases += 1
    nt, df, n_ch = 16, 8, 8                           # the 128-tap decimate-by-8 ring shape: chunks of two 256-output steps
    fin, fc = F(16, 2), F(16, 2)
    fa, fo = lossless_acc(fin, fc, 9), OUT16
    rng = np.random.default_rng(44)
    c = rand_raw(rng, fc, (nt * df,)) // 4
    orc = OraclePolyDec(nt, df, ofmt(fin), ofmt(fc), ofmt(fa), ofmt(fo), n_ch=n_ch)
    eng = None
    if GPU:
        eng = A.PolyDec(nt, df, fin, fc, fa, fo, n_channels=n_ch)
        eng.set_coeffs(c)
    for i, groups in enumerate((2048, 3, 512 + 16)):
        x = rand_raw(rng, fin, (n_ch, groups * df))
        yo = orc.run(c, x)
        if GPU:
            R.compare("polydec", i, host(eng.run(dev(x, fin))), yo)
            if i == 0:
                R.witness["polydec.path"] = eng.path


BATTERIES = {k[4:]: v for k, v in list(globals().items()) if k.startswith("bat_")}


def main(argv):
    names = [a for a in argv if not a.startswith("--")]
    if ORACLE_ONLY and not names:
        names = list(BATTERIES)
    if not names or any(n not in BATTERIES for n in names):
        sys.stderr.write("usage: knob_child.py [--oracle-only] BATTERY [BATTERY ...]\nbatteries: %s\n" % " ".join(BATTERIES))
        return 2
    if GPU:
        assert torch.cuda.is_available(), "knob_child.py needs the GPU (or --oracle-only)"
        torch.cuda.set_device(0)
    bad = 0
    for n in names:
        R = Result(n)
        t0 = time.perf_counter()
        BATTERIES[n](R)
        if GPU:
            torch.cuda.synchronize()
            print(R.line(), flush=True)
        else:
            print(json.dumps(dict(battery=n, cases=R.cases, oracle_seconds=round(time.perf_counter() - t0, 3))), flush=True)
        bad += R.mismatches
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
