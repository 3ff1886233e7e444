"""GPU parity tests, ac_mv_avg on byte rows (ACDSP_FLAG_IN_BYTES / ACDSP_FLAG_OUT_BYTES, mv_avg_s8.hip): the HIP engine reading int8 / uint8
rows -- and writing them under out_bytes -- against the CPU oracle, bit for bit.  No tolerances anywhere.

Types unless a case says otherwise: COEFF <16,8> (F = 8), ACC <40, .> with F_acc = F_in + 8 + ls (the linear class: the products add up
unshifted, ls = 2 bits of head room below them).  Five objects: the last workgroup of a launch is partly empty.  Every case on the byte-plane
kernel asserts path == "stream_s8"; every case that must stay off it asserts the kernel it runs on instead."""
import numpy as np
import pytest
import torch

import ac_dsp_amd as A
from helpers import ofmt, rand_fmt
from oracle import OracleFir, OracleMvAvg

pytestmark = pytest.mark.gpu

F = A.Fmt
N_OBJ = 5
FC = F(16, 8)
MODES = ["WIN", "MIRROR", "CLIP"]
FINS = [F(8, 4), F(8, 8, False), F(5, 5, False), F(1, 1, False)]
# (OUT_TYPE, out_bytes): 16-, 32- and 64-bit containers, then the three 1-byte forms
OUTS = [(F(16, 10, True, "RND", "SAT"), False), (F(24, 12, True, "TRN", "WRAP"), False), (F(40, 22), False),
        (F(8, 4, True, "RND", "SAT"), True), (F(8, 8, False, "TRN", "WRAP"), True), (F(4, 7, True, "RND", "SAT"), True)]


def acc_for(fin, ls=2, w=40, fc=FC):
    f_acc = (fin.W - fin.I) + (fc.W - fc.I) + ls
    return F(w, w - f_acc)


def weights(rng, taps, total=300):
    """TAPS signed weights with sum |c| <= total (total 256 = unit gain at F_coeff = 8), none above 32639 (the kernel's class)"""
    c = rng.integers(-(total // taps), total // taps + 1, size=taps, dtype=np.int64)
    c[taps // 2] += (total - np.abs(c).sum()) * (1 if rng.integers(0, 2) else -1)
    c[taps // 2] = min(c[taps // 2], 32639)
    assert np.abs(c).sum() <= total
    return c


def to_dev(x, dtype, misalign=0):
    """[rows][n] raw words -> device rows of `dtype` whose first element sits `misalign` elements behind a 512-byte boundary"""
    x = np.atleast_2d(x)
    pitch = (x.shape[1] + misalign + 63) // 64 * 64 + (64 if misalign else 0)
    buf = torch.zeros((x.shape[0], pitch), dtype=dtype, device="cuda")
    v = buf[:, misalign:misalign + x.shape[1]]
    v.copy_(torch.from_numpy(np.ascontiguousarray(x)).to(dtype))
    return v


def words(y):
    return y.cpu().numpy().astype(np.int64)


def same(y, yo, what=""):
    assert y.shape == yo.shape, (what, y.shape, yo.shape)
    bad = np.argwhere(y != yo)
    assert bad.size == 0, "%s: %d mismatches, first at %s: got %d want %d" % (what, len(bad), bad[0], y[tuple(bad[0])], yo[tuple(bad[0])])


def make(taps, mode, fin, fa, fo, c, out_bytes=False, in_bytes=True, n_obj=N_OBJ, fc=FC, max_sample=4096, **kw):
    eng = A.MvAvg(max_sample, taps, mode, fin, fc, fa, fo, n_objects=n_obj, in_bytes=in_bytes, out_bytes=out_bytes, **kw)
    eng.set_coeffs(c)
    return eng


def oracle(taps, mode, fin, fa, fo, n_obj=N_OBJ, fc=FC):
    return OracleMvAvg(taps, mode, ofmt(fin), ofmt(fc), ofmt(fa), ofmt(fo), n_obj=n_obj)


def case(taps, mode, fin, fa, fo, out_bytes, c, xs, n_sample, path="stream_s8", fc=FC, what="", **kw):
    """every x of xs is one call of the same handle; returns the handle"""
    eng = make(taps, mode, fin, fa, fo, c, out_bytes=out_bytes, fc=fc, **kw)
    orc = oracle(taps, mode, fin, fa, fo, fc=fc)
    assert eng.in_dtype == (torch.int8 if fin.S else torch.uint8)
    for k, x in enumerate(xs):
        y = eng.run(to_dev(x, eng.in_dtype), n_sample)
        assert y.dtype == eng.out_dtype and (not out_bytes or y.dtype == (torch.int8 if fo.S else torch.uint8)), (y.dtype, eng.out_dtype)
        assert eng.path == path, (eng.path, path, what)
        same(words(y), orc.run(c, x, n_sample), "%s call %d" % (what, k))
    return eng


# ---- 1. the fast-kernel grid -----------------------------------------------------------------------------------------------------------------
TAPS = [1, 3, 9, 31, 33, 35, 63, 65]            # 33 | 35: one | two K blocks
FRAMES = [(80, 1), (80, 3), (512, 1), (512, 3), (528, 1), (528, 3), (1040, 1), (1040, 3)]


def _grid():
    """a sampled product: 64 cases in which every value of every parameter and every (taps, mode) pair occurs; strides coprime to the list lengths"""
    out = []
    for i in range(64):
        taps, mode = TAPS[i % 8], MODES[(i // 8) % 3]
        n, fr = FRAMES[(3 * i + i // 8) % 8]
        fin = FINS[(i + i // 8) % 4]
        fo, ob = OUTS[(i + 3 * (i // 8)) % 6]
        out.append(pytest.param(i, taps, mode, n, fr, fin, fo, ob, id="%d-T%d-%s-%dx%d-i%d%s-o%d%s" % (i, taps, mode, n, fr, fin.W, "s" if fin.S else "u", fo.W, "b" if ob else "")))
    return out


def test_the_sampled_grid_covers_every_value():
    g = [p.values for p in _grid()]
    assert {v[1] for v in g} == set(TAPS) and {v[2] for v in g} == set(MODES) and {(v[3], v[4]) for v in g} == set(FRAMES)
    assert {(v[5].W, v[5].S) for v in g} == {(f.W, f.S) for f in FINS} and {(v[6].W, v[7]) for v in g} == {(f.W, b) for f, b in OUTS}
    assert {(v[1], v[2]) for v in g} == {(t, m) for t in TAPS for m in MODES}


@pytest.mark.parametrize("i,taps,mode,n,frames,fin,fo,out_bytes", _grid())
def test_fast_kernel_grid(i, taps, mode, n, frames, fin, fo, out_bytes):
    rng = np.random.default_rng(1000 + i)
    c = weights(rng, taps, 300 if i % 3 else 32767)
    xs = [rand_fmt(rng, fin, (N_OBJ, n * frames)) for _ in range(2)]
    case(taps, mode, fin, acc_for(fin), fo, out_bytes, c, xs, n, what="grid %d" % i)


# ---- 2. full scale -----------------------------------------------------------------------------------------------------------------------------
def _full_scale_rows(fin, n, frames):
    lo, hi = (-(1 << (fin.W - 1)), (1 << (fin.W - 1)) - 1) if fin.S else (0, (1 << fin.W) - 1)
    x = np.empty((N_OBJ, n * frames), dtype=np.int64)
    x[0], x[1] = lo, hi
    x[2] = np.where(np.arange(n * frames) % 2 == 0, lo, hi)
    x[3] = np.where((np.arange(n * frames) // n) % 2 == 0, lo, hi)
    x[4] = np.where(np.arange(n * frames) % 2 == 0, hi, lo)
    return x


def _full_scale_sets(taps):
    one = np.full(taps, 32767 // taps, dtype=np.int64)
    one[taps // 2] += 32767 - one.sum()
    alt = one * np.where(np.arange(taps) % 2 == 0, 1, -1)
    return {"one_sign": one, "negative": -one, "alternating": alt, "all_127": np.full(taps, 127, dtype=np.int64)}


@pytest.mark.parametrize("fin", [F(8, 4), F(8, 8, False)], ids=["signed", "unsigned"])
@pytest.mark.parametrize("cset", ["one_sign", "negative", "alternating", "all_127"])
@pytest.mark.parametrize("past", [0, 1], ids=["last_safe_bit", "one_bit_further"])
def test_full_scale(fin, cset, past):
    """A 32-bit accumulator.  |sum c x| <= 32767 * 2^7 < 2^22 on signed samples (32767 * 2^8 < 2^23 on unsigned ones), so the accumulator
    holds sum * 2^ls without wrapping up to ls = 32 - 1 - 22 = 9 (8): the 32-bit epilogue's last safe bit.  One bit further the product of
    full-scale rows and a one-signed set wraps the accumulator, which only the 64-bit form models."""
    taps, mode, n, frames = 33, "MIRROR", 528, 3
    ls = (9 if fin.S else 8) + past
    fa = acc_for(fin, ls=ls, w=32)
    c = _full_scale_sets(taps)[cset]
    assert np.abs(c).sum() <= 32767 and c.max() <= 32639
    x = _full_scale_rows(fin, n, frames)
    for fo, ob in ((F(16, 12, True, "RND", "SAT"), False), (F(8, 11, True, "RND", "SAT"), True)):
        case(taps, mode, fin, fa, fo, ob, c, [x], n, what="%s ls %d" % (cset, ls))
    if past and cset in ("one_sign", "negative"):
        yo = oracle(taps, mode, fin, acc_for(fin, ls=ls, w=48), F(40, 24)).run(c, x, n)      # the same sums in an accumulator that holds them
        yw = oracle(taps, mode, fin, fa, F(40, 24)).run(c, x, n)
        assert (yo != yw).any(), "the case does not wrap the 32-bit accumulator"


# ---- 3. digits ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("taps", [9, 33, 35, 65])
def test_coefficient_digits(mode, taps):
    rng = np.random.default_rng(3000 + taps)
    fin, n, frames = F(8, 4), 528, 2
    fa, fo = acc_for(fin), F(24, 12, True, "RND", "SAT")
    x = [rand_fmt(rng, fin, (N_OBJ, n * frames))]
    sets = {"one plane": rng.integers(-128, 128, size=taps, dtype=np.int64), "one plane, extremes": np.where(np.arange(taps) % 2 == 0, -128, 127).astype(np.int64)}
    for v in (128, 255, -129, 256, 32639):
        for pos in (0, taps // 2, taps - 1):
            c = np.zeros(taps, dtype=np.int64)
            c[pos] = v
            if taps > 1:
                c[(pos + 1) % taps] = 1                                  # a second tap: a misplaced digit cannot hide behind a lone one
            sets["%d at %d" % (v, pos)] = c
    for name, c in sets.items():
        case(taps, mode, fin, fa, fo, False, c, x, n, what=name)


def test_a_high_digit_in_the_second_k_block_only():
    """65 taps under AC_WIN: tap 64 lies in the second K block of every row (64 = 64 b + kk - s needs b = 1), so with one-byte weights everywhere
    else the first block's high-digit fragments are all zero"""
    rng = np.random.default_rng(77)
    fin, n = F(8, 8, False), 528
    c = rng.integers(-100, 101, size=65, dtype=np.int64)
    c[64] = 20000
    for fo, ob in ((F(15, 15, False, "RND", "SAT"), False), (F(8, 15, False, "RND", "SAT"), True)):
        case(65, "WIN", fin, acc_for(fin), fo, ob, c, [rand_fmt(rng, fin, (N_OBJ, 2 * n))], n)


# ---- 4. what declines stays exact -------------------------------------------------------------------------------------------------------------
def test_declines_stay_exact():
    rng = np.random.default_rng(4)
    fin, fo8, fo16 = F(8, 4), F(8, 4, True, "RND", "SAT"), F(16, 8, True, "RND", "SAT")
    fa = acc_for(fin)
    n = 512
    x = [rand_fmt(rng, fin, (N_OBJ, 2 * n))]
    c9 = weights(rng, 9)
    # the per-tap class, d = F_acc - F_in < sh = F_coeff: every product loses bits before it is added (the benchmark's COEFF <16,2> and OUT
    # <16,8,RND,SAT> on samples narrowed to <8,0>, with the accumulator <32,16> of test_mvavg_gpu's per-tap rows: d = 8 < 14)
    cb = np.round(np.hanning(11)[1:-1] / np.hanning(11).sum() * 2.0 ** 14).astype(np.int64)
    for ob, fo in ((False, F(16, 8, True, "RND", "SAT")), (True, F(8, 0, True, "RND", "SAT"))):
        case(9, "MIRROR", F(8, 0), F(32, 16), fo, ob, cb, [rand_fmt(rng, F(8, 0), (N_OBJ, 2 * n))], n, path="int64_sums", fc=F(16, 2), what="per tap")
    # ... while the benchmark's own accumulator <40,18> on those samples is the linear class (d = 14 = sh)
    case(9, "MIRROR", F(8, 0), F(40, 18), F(16, 8, True, "RND", "SAT"), False, cb, [rand_fmt(rng, F(8, 0), (N_OBJ, 2 * n))], n, fc=F(16, 2), what="bench types")
    # 67 taps
    case(67, "MIRROR", fin, fa, fo8, True, weights(rng, 67), x, n, path="int64_sums", what="67 taps")
    # frames of 24 and 1000 samples: multiples of 8, not of 16
    for ns in (24, 1000):
        case(9, "CLIP", fin, fa, fo8, True, c9, [rand_fmt(rng, fin, (N_OBJ, 2 * ns))], ns, path="int64_sums", what="n_sample %d" % ns)
    # ACDSP_FLAG_FORCE_GENERIC
    case(9, "MIRROR", fin, fa, fo8, True, c9, x, n, path="exact_order", force_generic=True, what="force_generic")
    # an AC_SAT accumulator that does saturate: <12,4> holds +-8 in F = 8 + ... bits; sums of gain 8 on +-8 samples reach +-64
    fa_sat = F(4 + 14, 4, True, "TRN", "SAT")
    csat = np.full(9, 227, dtype=np.int64)
    xs = _full_scale_rows(fin, n, 2)
    eng = case(9, "MIRROR", fin, fa_sat, fo16, False, csat, [xs], n, path="exact_order", what="saturating accumulator")
    yo = oracle(9, "MIRROR", fin, fa_sat, fo16).run(csat, xs, n)
    yw = oracle(9, "MIRROR", fin, F(18, 4), fo16).run(csat, xs, n)
    assert (yo != yw).any(), "the accumulator does not saturate"
    del eng
    # ... and one that cannot: the same kernel as a wrapping accumulator
    case(9, "MIRROR", fin, F(40, 22, True, "TRN", "SAT"), fo8, True, c9, x, n, what="sat-free accumulator")


def test_an_input_row_one_byte_off_the_boundary_declines():
    rng = np.random.default_rng(41)
    fin, fo = F(8, 4), F(8, 4, True, "RND", "SAT")
    c, n = weights(rng, 9), 512
    x = rand_fmt(rng, fin, (N_OBJ, 2 * n))
    eng = make(9, "MIRROR", fin, acc_for(fin), fo, c, out_bytes=True)
    xd = to_dev(x, torch.int8, misalign=1)
    assert xd.data_ptr() % 16 == 1
    y = eng.run(xd, n)
    assert eng.path == "int64_sums", eng.path
    same(words(y), oracle(9, "MIRROR", fin, acc_for(fin), fo).run(c, x, n))
    # the same rows with a pitch that is no multiple of 16
    xd = to_dev(x, torch.int8)
    xp = torch.zeros((N_OBJ, 2 * n + 8), dtype=torch.int8, device="cuda")[:, :2 * n]
    xp.copy_(xd)
    assert xp.data_ptr() % 16 == 0 and xp.stride(0) % 16 == 8
    y = eng.run(xp, n)
    assert eng.path == "int64_sums", eng.path
    same(words(y), oracle(9, "MIRROR", fin, acc_for(fin), fo).run(c, x, n))


@pytest.mark.parametrize("mode", ["MIRROR", "WIN"])
def test_an_output_row_one_byte_off_the_boundary_takes_element_stores(mode):
    rng = np.random.default_rng(42)
    fin, fo = F(8, 8, False), F(8, 8, False, "RND", "SAT")
    c, n = weights(rng, 9, 256), 528
    x = rand_fmt(rng, fin, (N_OBJ, 3 * n))
    eng = make(9, mode, fin, acc_for(fin), fo, c, out_bytes=True)
    no = eng.out_per_frame(n) * 3
    buf = torch.full((N_OBJ, no + 64), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[:, 1:1 + no]
    assert out.data_ptr() % 16 == 1
    y = eng.run(to_dev(x, torch.uint8), n, out=out)
    assert eng.path == "stream_s8", eng.path
    same(words(y), oracle(9, mode, fin, acc_for(fin), fo).run(c, x, n))
    b = words(buf)
    assert (b[:, 0] == 0xA5).all() and (b[:, 1 + no:] == 0xA5).all()


# ---- 5. confinement ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,taps", [("MIRROR", 35), ("WIN", 9), ("WIN", 3), ("CLIP", 65)])
@pytest.mark.parametrize("out_bytes", [True, False], ids=["out1", "out2"])
def test_no_byte_outside_the_output_rows_is_written(mode, taps, out_bytes):
    """sentinel rows with a pitch beyond the row, the rows 16 bytes into them; AC_WIN rows are shorter than the input (9 taps: whole 8-output groups
    on the vector stores; 3 taps: 526 outputs per frame on the element stores)"""
    rng = np.random.default_rng(50 + taps)
    fin = F(8, 4)
    fo = F(8, 4, True, "RND", "SAT") if out_bytes else F(16, 8, True, "RND", "SAT")
    c, n, frames = weights(rng, taps, 256), 528, 3
    x = rand_fmt(rng, fin, (N_OBJ, n * frames))
    eng = make(taps, mode, fin, acc_for(fin), fo, c, out_bytes=out_bytes)
    no = eng.out_per_frame(n) * frames
    sentinel = 0x5A if out_bytes else 0x5A5A
    lead = 16 if out_bytes else 8                                         # elements = 16 bytes
    buf = torch.full((N_OBJ + 1, no + 2 * lead + 40), sentinel, dtype=eng.out_dtype, device="cuda")
    out = buf[:N_OBJ, lead:lead + no]
    y = eng.run(to_dev(x, torch.int8), n, out=out)
    assert eng.path == "stream_s8" and y.shape == (N_OBJ, no)
    same(words(y), oracle(taps, mode, fin, acc_for(fin), fo).run(c, x, n))
    b = words(buf)
    assert (b[:N_OBJ, :lead] == sentinel).all() and (b[:N_OBJ, lead + no:] == sentinel).all() and (b[N_OBJ] == sentinel).all()


# ---- 6. equivalence with int16 containers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fin,fo", [(F(8, 4), F(8, 4, True, "RND", "SAT")), (F(8, 8, False), F(8, 8, False, "TRN", "WRAP"))], ids=["signed", "unsigned"])
@pytest.mark.parametrize("taps,mode", [(9, "MIRROR"), (35, "WIN")])
def test_the_same_values_in_int16_containers_give_the_same_words(fin, fo, taps, mode):
    rng = np.random.default_rng(60 + taps)
    c, n = weights(rng, taps, 256), 1040
    x = rand_fmt(rng, fin, (N_OBJ, 2 * n))
    plain = make(taps, mode, fin, acc_for(fin), fo, c, in_bytes=False)
    assert plain.in_dtype == torch.int16 and plain.out_dtype == torch.int16
    yw = words(plain.run(to_dev(x, torch.int16), n))
    assert plain.path in ("stream", "stream_mfma"), plain.path
    for ob in (False, True):
        eng = make(taps, mode, fin, acc_for(fin), fo, c, out_bytes=ob)
        y = eng.run(to_dev(x, eng.in_dtype), n)
        assert eng.path == "stream_s8" and y.element_size() == (1 if ob else 2)
        same(words(y), yw, "out_bytes %s" % ob)


# ---- 7. chain: mv_avg -> FIR without a narrowing pass --------------------------------------------------------------------------------------
def test_a_byte_output_row_feeds_a_byte_fir_as_it_is():
    rng = np.random.default_rng(7)
    fin, mid = F(8, 4), F(8, 2, True, "RND", "SAT")                         # the FIR's IN_TYPE <8,2> is the moving average's OUT_TYPE
    c, n, n_taps = weights(rng, 9, 256), 1040, 63
    x = rand_fmt(rng, fin, (N_OBJ, 2 * n))
    mv = make(9, "MIRROR", fin, acc_for(fin), mid, c, out_bytes=True)
    ffc, ffa, ffo = F(16, 2), F(48, 28), F(16, 6, True, "RND", "SAT")
    h = rng.integers(-2000, 2001, size=n_taps, dtype=np.int64)
    fir = A.Fir(n_taps, "SHIFT_REG", F(8, 2), ffc, ffa, ffo, n_channels=N_OBJ, kind="load", in_bytes=True)
    fir.set_coeffs(h)
    y1 = mv.run(to_dev(x, torch.int8), n)
    assert mv.path == "stream_s8" and y1.dtype == torch.int8 == fir.in_dtype
    y2 = fir.run(y1)
    m = oracle(9, "MIRROR", fin, acc_for(fin), mid).run(c, x, n)
    same(words(y1), m, "stage 1")
    same(words(y2), OracleFir(n_taps, "SHIFT_REG", ofmt(F(8, 2)), ofmt(ffc), ofmt(ffa), ofmt(ffo), n_ch=N_OBJ).run(h, m), "stage 2")


# ---- 8. the other entry points ---------------------------------------------------------------------------------------------------------------
def test_clone_of_a_flagged_handle():
    rng = np.random.default_rng(8)
    fin, fo = F(8, 8, False), F(8, 8, False, "RND", "SAT")
    c, n = weights(rng, 33, 256), 512
    x = rand_fmt(rng, fin, (N_OBJ, 2 * n))
    eng = make(33, "CLIP", fin, acc_for(fin), fo, c, out_bytes=True)
    twin = eng.clone()
    assert twin.in_bytes and twin.out_bytes and twin.in_dtype == torch.uint8 and twin.out_dtype == torch.uint8
    assert A._lib.lib.acdsp_mvavg_in_elem_bytes(twin._h) == 1 and A._lib.lib.acdsp_mvavg_out_elem_bytes(twin._h) == 1
    eng.close()
    y = twin.run(to_dev(x, torch.uint8), n)
    assert twin.path == "stream_s8"
    same(words(y), oracle(33, "CLIP", fin, acc_for(fin), fo).run(c, x, n))


@pytest.mark.parametrize("fin,in_bytes,paths", [(F(16, 8), False, ["stream", "stream32", "stream"]), (F(8, 4), True, ["stream_s8", "int64_sums", "stream_s8"])], ids=["int16", "bytes"])
def test_a_new_coefficient_set_replans_a_live_handle(fin, in_bytes, paths):
    """What a handle decides per coefficient set is rebuilt by every set_coeffs: a normalised window (sum |c| = 2^14: the streaming / byte kernel), then all
    taps 8191 (sum |c| > 32767: off both, on to the 32-bit sliding window / the int64 sums), then the window again -- every run against the oracle, and a
    clone taken under the second set decides as its source does."""
    taps, n, n_obj = 9, 1024, 2
    fc, fa, fo = F(16, 2), F(40, 18), F(16, 8, True, "RND", "SAT")
    w = np.hanning(taps + 2)[1:-1]
    set_a = np.round(w / w.sum() * 2.0 ** 14).astype(np.int64)
    set_a[taps // 2] += 2 ** 14 - set_a.sum()
    set_b = np.full(taps, 8191, dtype=np.int64)
    x = rand_fmt(np.random.default_rng(41), fin, (n_obj, 2 * n))
    orc = oracle(taps, "MIRROR", fin, fa, fo, n_obj=n_obj, fc=fc)
    want = {"a": orc.run(set_a, x, n), "b": orc.run(set_b, x, n)}
    eng = A.MvAvg(4096, taps, "MIRROR", fin, fc, fa, fo, n_objects=n_obj, in_bytes=in_bytes)
    xd = to_dev(x, eng.in_dtype)
    for k, (name, c) in enumerate((("a", set_a), ("b", set_b), ("a", set_a))):
        eng.set_coeffs(c)
        y = words(eng.run(xd, n))
        assert eng.path == paths[k], (k, eng.path)
        same(y, want[name], "set %s, run %d" % (name, k))
        if k == 1:
            twin = eng.clone()
            assert twin.path == eng.path
            same(words(twin.run(xd, n)), want["b"], "clone under set b")
            assert twin.path == paths[1], twin.path
            twin.close()


@pytest.mark.parametrize("fin,fo", [(F(8, 4), F(8, 4, True, "RND", "SAT")), (F(8, 8, False), F(8, 8, False, "RND", "SAT"))], ids=["int8", "uint8"])
def test_run_host_on_numpy_byte_rows(fin, fo):
    rng = np.random.default_rng(81)
    c, n = weights(rng, 9, 256), 512
    x = rand_fmt(rng, fin, (N_OBJ, 2 * n))
    want = oracle(9, "MIRROR", fin, acc_for(fin), fo).run(c, x, n)
    for ob in (True, False):
        eng = make(9, "MIRROR", fin, acc_for(fin), fo, c, out_bytes=ob)
        y = eng.run_host(x.astype(np.int8 if fin.S else np.uint8), n)
        assert y.dtype == ((np.int8 if fo.S else np.uint8) if ob else np.int16) and eng.path == "stream_s8"
        same(y.astype(np.int64), want, "out_bytes %s" % ob)


def test_node_with_two_shards_on_device_0():
    rng = np.random.default_rng(82)
    fin, fo = F(8, 4), F(8, 4, True, "RND", "SAT")
    c, n = weights(rng, 9, 256), 512
    x = rand_fmt(rng, fin, (N_OBJ, 2 * n))
    node = A.NodeMvAvg(4096, 9, "MIRROR", fin, FC, acc_for(fin), fo, N_OBJ, [0, 0], in_bytes=True, out_bytes=True)
    node.set_coeffs(c)
    assert node.in_dtype == torch.int8 and node.out_dtype == torch.int8
    xs = [to_dev(x[lo:hi], torch.int8).contiguous() for lo, hi in node.slices]
    ys = node.run(xs, n)
    assert all(y.dtype == torch.int8 for y in ys)
    same(np.concatenate([words(y) for y in ys]), oracle(9, "MIRROR", fin, acc_for(fin), fo).run(c, x, n))
    assert all(A._lib.lib.acdsp_mvavg_path(node.shard_handle(s)) == 5 for s in range(node.n_shards))


# ---- 9. graph capture --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_bytes", [True, False], ids=["out1", "out2"])
def test_capture_and_three_replays(out_bytes):
    """stateless: one captured call of the path-5 kernel, replayed on changed input contents (after test_graph_paths_gpu's mv_avg case)"""
    rng = np.random.default_rng(9)
    fin = F(8, 4)
    fo = F(8, 4, True, "RND", "SAT") if out_bytes else F(16, 8, True, "RND", "SAT")
    taps, mode, n, frames = 17, "MIRROR", 1024, 4
    c = weights(rng, taps, 256)
    eng = make(taps, mode, fin, acc_for(fin), fo, c, out_bytes=out_bytes)
    orc = oracle(taps, mode, fin, acc_for(fin), fo)
    side = torch.cuda.Stream()
    x0 = rand_fmt(rng, fin, (N_OBJ, n * frames))
    xd = to_dev(x0, torch.int8)
    with torch.cuda.stream(side):
        y = eng.run(xd, n)                                                # an eager call on the capture stream in front
    side.synchronize()
    same(words(y), orc.run(c, x0, n), "eager call in front")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        y = eng.run(xd, n)
        assert eng.path == "stream_s8"
    torch.cuda.synchronize()
    for r in range(3):
        x = rand_fmt(np.random.default_rng(900 + r), fin, (N_OBJ, n * frames))
        xd.copy_(torch.from_numpy(x).to(torch.int8))
        y.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        same(words(y), orc.run(c, x, n), "replay %d" % r)
    x = rand_fmt(rng, fin, (N_OBJ, n * frames))
    same(words(eng.run(to_dev(x, torch.int8), n)), orc.run(c, x, n), "eager call behind the replays")


# ---- 10. runs of tiles per wave ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tpw", [3, 7, 64])
def test_runs_of_tiles_per_wave(tpw):
    """By itself the launcher gives a wave more than one tile only from 16384 tiles on (8 MB rows).  ACDSP_MVAVG_TPW is read once per process, so a
    child (tests/mvavg_bytes_tpw_child.py) runs small rows with 3, 7 and 64 tiles per wave: the four register sets of tiles in flight wrap, runs
    end inside frames and objects, and the last wave of a launch is short."""
    import os
    import subprocess
    import sys
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mvavg_bytes_tpw_child.py")
    env = {k: v for k, v in os.environ.items() if not k.startswith("ACDSP_") or k in ("ACDSP_LIB", "ACDSP_ORACLE_LIB")}
    env["ACDSP_MVAVG_TPW"] = str(tpw)
    p = subprocess.run([sys.executable, child], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0 and out.rstrip().endswith("OK"), out[-3000:]
