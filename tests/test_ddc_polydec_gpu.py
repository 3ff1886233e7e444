"""GPU parity tests, DDC with a decimating second stage: acdsp_ddc_create_polydec (ac_cic_dec_full -> ac_poly_dec in one fused kernel, and on the
two stage kernels) against OracleCic -> OraclePolyDec on whole groups, the pending words queued by the test helper (ddc_polydec_ref.py).
Every comparison is exact."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

import ac_dsp_amd as A
from ac_dsp_amd import _lib as L
from ddc_polydec_ref import oracle_cascade, oracle_mid, polydec_coeffs, run_stream
from helpers import refused_under_capture, windowed_sinc

pytestmark = pytest.mark.gpu

# the config-5 class: R 16 M 1 N 5 on <16,1> samples, <36,21> words, NTAPS 64 x DF 2 = a 128-tap prototype in <16,1>, sums in <60,30>
CFG5 = dict(R=16, M=1, N=5, cin=A.Fmt(16, 1), n_taps=64, df=2, fc=A.Fmt(16, 1), fa=A.Fmt(60, 30))
FO = A.Fmt(24, 9, True, "RND", "SAT")
CHUNK = 4 * 256   # outputs per chunk of the fused launch (launch_cascade_dec: 8 / DF steps of 256)
FUSED_RATES = [16, 17]   # decimation rates of the fused class the phase test walks: config 5's, and its neighbour R 17 (INT_TYPE <37,22>)


def make(g, fo, n_ch, **kw):
    d = A.DdcPolyDec(g["R"], g["M"], g["N"], g["cin"], g["n_taps"], g["df"], g["fc"], g["fa"], fo, n_channels=n_ch, **kw)
    return d


def ref(g, fo, mid, c, x, splits=None, u=None):
    return oracle_cascade(g["R"], g["M"], g["N"], g["cin"], mid, g["n_taps"], g["df"], g["fc"], g["fa"], fo, c, x, splits, u)


_shared = {}


def cfg5_stream():
    """3 channels, three complete chunks + a ragged tail of final outputs, an odd word count; the decimator's words computed once"""
    if not _shared:
        rng = np.random.default_rng(41)
        n = 16 * (2 * (3 * CHUNK + 256 + 77) + 1)
        x = rng.integers(-32768, 32768, size=(3, n))
        _shared["x"] = x
        _shared["u"] = oracle_mid(16, 1, 5, CFG5["cin"], A.Fmt(36, 21), x)
        _shared["c"] = polydec_coeffs(64, 2, CFG5["fc"])
    return _shared["x"], _shared["u"], _shared["c"]


# 1. both limb epilogues (OUT <= 31 bits: AC_SAT with the clamp in the high limb, AC_WRAP) and the 64-bit one (32-bit OUT)
@pytest.mark.parametrize("fo", [A.Fmt(24, 9, True, "RND", "SAT"), A.Fmt(24, 9, True, "TRN", "WRAP"), A.Fmt(32, 12, True, "RND", "WRAP"),
                                A.Fmt(20, 3, True, "TRN", "SAT"), A.Fmt(31, 12, True, "RND", "SAT"), A.Fmt(18, 17, True, "RND", "SAT"),
                                A.Fmt(30, 29, True, "RND", "WRAP")])
def test_fused_polydec_cascade_matches_the_oracle_cascade(fo):
    g = CFG5
    x, u, c = cfg5_stream()
    ddc = make(g, fo, 3)
    assert (ddc.int_type.W, ddc.int_type.I) == (36, 21)
    ddc.set_coeffs(c)
    assert ddc.path == "fused"
    y = run_stream(ddc, x)
    yo = ref(g, fo, ddc.int_type, c, x, u=u)
    assert yo.shape[1] == u.shape[1] // 2 and yo.shape[1] >= 3 * CHUNK + 256
    assert y.shape == yo.shape and np.array_equal(y, yo)


# 2. odd word counts between calls (the queue is non-empty), a burst below one step, a burst without output; reset
def test_fused_streaming_carries_the_queue_across_calls():
    g = CFG5
    rng = np.random.default_rng(42)
    # words per burst: 301 (1 waits), 1300 (1 waits), ONE word that meets the waiting one, one word that waits alone (no output), 37 -- below a
    # step of 256 outputs --, two chunks and three words, the rest
    splits = np.cumsum([16 * 301, 16 * 1300, 16, 16, 16 * 37, 16 * 2 * CHUNK + 48]).tolist()
    n = splits[-1] + 16 * 801
    x = rng.integers(-32768, 32768, size=(2, n))
    c = polydec_coeffs(g["n_taps"], g["df"], g["fc"])
    ddc = make(g, FO, 2)
    ddc.set_coeffs(c)
    assert ddc.path == "fused"
    counts = []
    y = run_stream(ddc, x, splits, counts)
    yo = ref(g, FO, ddc.int_type, c, x, splits)
    assert counts[:4] == [150, 650, 1, 0], counts
    assert np.array_equal(y, yo)
    ddc.reset()
    assert np.array_equal(run_stream(ddc, x[:, :splits[1]], splits[:1]), yo[:, :800])


# 3. the two stage kernels: other rates and DF, the config-5 class at DF 3, byte rows
def test_two_kernel_shapes_match_and_say_so():
    rng = np.random.default_rng(43)
    # R 8 on <32,16> samples, NTAPS 21 x DF 3
    g = dict(R=8, M=1, N=5, cin=A.Fmt(32, 16), n_taps=21, df=3, fc=A.Fmt(16, 1), fa=A.Fmt(64, 31))
    fo = A.Fmt(32, 16, True, "RND", "SAT")
    splits = [8 * 1000, 8 * 1001, 8 * 2002]   # 1000 words: 1 waits; 1 more: 2 wait; 1001 more: 1003 = 334 * 3 + 1
    x = rng.integers(-(1 << 31), 1 << 31, size=(2, 8 * 2502))
    c = polydec_coeffs(21, 3, g["fc"])
    ddc = make(g, fo, 2)
    ddc.set_coeffs(c)
    assert ddc.path == "two_kernels"
    counts = []
    y = run_stream(ddc, x, splits, counts)
    assert counts == [333, 0, 334, 167], counts
    assert np.array_equal(y, ref(g, fo, ddc.int_type, c, x, splits))
    # the config-5 class with DF 3: outside the fused class
    g3 = dict(CFG5, n_taps=40, df=3)
    x = rng.integers(-32768, 32768, size=(2, 16 * 4001))
    c = polydec_coeffs(40, 3, g3["fc"])
    ddc = make(g3, FO, 2)
    ddc.set_coeffs(c)
    assert ddc.path == "two_kernels"
    sp = [16 * 1000, 16 * 1001]
    assert np.array_equal(run_stream(ddc, x, sp), ref(g3, FO, ddc.int_type, c, x, sp))
    # byte rows: <8,1> samples in 1-byte containers, the decimator stage as under ACDSP_FLAG_IN_BYTES
    g8 = dict(CFG5, cin=A.Fmt(8, 1))
    x = rng.integers(-128, 128, size=(2, 16 * 3001))
    c = polydec_coeffs(64, 2, g8["fc"])
    ddc = make(g8, FO, 2, in_bytes=True)
    ddc.set_coeffs(c)
    assert ddc.path == "two_kernels" and ddc.in_dtype == torch.int8
    sp = [16 * 1001]
    assert np.array_equal(run_stream(ddc, x, sp), ref(g8, FO, ddc.int_type, c, x, sp))


# 4. state blobs and clones, taken with words waiting -- one at DF 2 and 3, 37 at DF 40: more than a 32-word row --; refusals of foreign blobs
@pytest.mark.parametrize("mode,g,words", [("fused", CFG5, 1501), ("two_kernels", dict(CFG5, n_taps=40, df=3), 1501),
                                          ("two_kernels", dict(CFG5, n_taps=4, df=40), 40 * 30 + 37)], ids=["fused", "two_kernels", "two_kernels_df40"])
def test_state_and_clone_continue_with_a_non_empty_queue(mode, g, words):
    rng = np.random.default_rng(44)
    cut = 16 * words
    x = rng.integers(-32768, 32768, size=(2, cut + 16 * 1200))
    c = polydec_coeffs(g["n_taps"], g["df"], g["fc"])
    yo = ref(g, FO, A.Fmt(36, 21), c, x, [cut])
    n0 = words // g["df"]
    assert words % g["df"] == (37 if g["df"] == 40 else 1)
    ddc = make(g, FO, 2)
    ddc.set_coeffs(c)
    assert ddc.path == mode
    assert np.array_equal(run_stream(ddc, x[:, :cut]), yo[:, :n0])
    blob = ddc.state()
    twin = ddc.clone()
    fresh = make(g, FO, 2)
    fresh.set_coeffs(c)
    fresh.set_state(blob)
    # refusals: another channel count, a truncated blob, a FIR cascade's blob and the reverse -- each leaves the handle as it was
    other = make(g, FO, 3)
    other.set_coeffs(c)
    fir = A.Ddc(g["R"], g["M"], g["N"], g["cin"], 127, "SHIFT_REG", g["fc"], g["fa"], FO, n_channels=2,
                flags=0 if mode == "fused" else L.FLAG_FORCE_GENERIC)
    fir.set_coeffs(windowed_sinc(127, 0.2, g["fc"]))
    assert fir.path == mode
    keep = fresh.state()
    assert keep == blob
    bad_blobs = [other.state(), blob[:-8], fir.state()]
    if mode == "two_kernels":
        # the outer header fits, the CIC blob inside is good and the ac_poly_dec blob behind it is not: the CIC state must be put back.  The
        # donor stands elsewhere in the stream, so a half-applied blob would show
        donor = make(g, FO, 2)
        donor.set_coeffs(c)
        run_stream(donor, x[:, :16 * (words - g["df"])])
        dblob = bytearray(donor.state())
        n_ch, eb, per = struct.unpack_from("<IIQ", dblob, 64 + 16)           # the CIC blob's header: n_channels, elem_bytes, per_channel
        inner = 64 + 64 + n_ch * eb * per                                    # ... behind it the ac_poly_dec blob
        assert bytes(dblob[inner:inner + 8]) == b"ACDSPST1"
        dblob[inner] ^= 0xFF
        bad_blobs.append(bytes(dblob))
    for bad in bad_blobs:
        with pytest.raises(A.AcdspError) as e:
            fresh.set_state(bad)
        assert e.value.code == 1
        assert fresh.state() == keep
    with pytest.raises(A.AcdspError) as e:
        fir.set_state(blob)
    assert e.value.code == 1
    for h in (ddc, twin, fresh):
        assert h.path == mode
        assert np.array_equal(run_stream(h, x[:, cut:]), yo[:, n0:])


# 5. the composite against separately run Cic + PolyDec handles, the leftover words queued by hand
@pytest.mark.parametrize("g", [CFG5, dict(CFG5, n_taps=40, df=3)], ids=["fused", "two_kernels"])
def test_composite_equals_separate_cic_and_polydec_handles(g):
    rng = np.random.default_rng(45)
    splits = [16 * 701, 16 * 1402, 16 * 1403]
    x = rng.integers(-32768, 32768, size=(2, 16 * 3000))
    c = polydec_coeffs(g["n_taps"], g["df"], g["fc"])
    ddc = make(g, FO, 2)
    ddc.set_coeffs(c)
    y = run_stream(ddc, x, splits)
    mid = ddc.int_type
    cic = A.Cic(False, g["R"], g["M"], g["N"], g["cin"], mid, n_channels=2)
    pd = A.PolyDec(g["n_taps"], g["df"], mid, g["fc"], g["fa"], FO, n_channels=2)
    pd.set_coeffs(c)
    pend = torch.zeros((2, 0), dtype=torch.int64, device="cuda")
    outs = []
    for a, b in zip([0] + splits, splits + [x.shape[1]]):
        u = cic.run(torch.from_numpy(x[:, a:b].copy()).to(torch.int16).cuda())
        w = torch.cat([pend, u], dim=1)
        k = w.shape[1] // g["df"] * g["df"]
        if k:
            wk = torch.zeros((2, (k + 15) // 16 * 16), dtype=torch.int64, device="cuda")   # rows readable up to a whole slot
            wk[:, :k] = w[:, :k]
            outs.append(pd.run(wk[:, :k]).cpu().numpy().astype(np.int64))
        pend = w[:, k:].clone()
    assert np.array_equal(y, np.concatenate(outs, axis=1))


# 6. the ordered refusals of acdsp_ddc_create_polydec, each in front of the ones behind it
def test_refusals_come_in_the_documented_order():
    it = A.Fmt(36, 21)
    f16, fa = A.Fmt(16, 1), A.Fmt(60, 30)

    def cd(**kw):
        d = dict(interp=0, R=16, M=1, N=5, n_channels=2, fin=f16, fout=it, device=0, flags=0)
        d.update(kw)
        return L.CicDesc(d["interp"], d["R"], d["M"], d["N"], d["n_channels"], d["fin"], d["fout"], d["device"], d["flags"])

    def pd(**kw):
        d = dict(n_taps=64, df=2, n_channels=2, fin=it, fcoeff=f16, facc=fa, fout=FO, device=0, flags=0)
        d.update(kw)
        return L.PolyDecDesc(d["n_taps"], d["df"], d["n_channels"], d["fin"], d["fcoeff"], d["facc"], d["fout"], d["device"], d["flags"])

    def create(c, p, flags=0):
        h = C.c_void_p()
        rc = L.lib.acdsp_ddc_create_polydec(C.byref(c) if c is not None else None, C.byref(p) if p is not None else None, flags, C.byref(h))
        msg = L.lib.acdsp_last_error().decode()
        if rc == 0:
            L.lib.acdsp_ddc_destroy(h)
        return rc, msg

    EINVAL, EUNSUPPORTED = 1, 2
    # every later descriptor below also carries the faults of the items behind it: the earlier refusal must win
    bad_all = dict(interp=1, n_channels=5, fout=A.Fmt(40, 21))
    assert create(None, pd())[0] == EINVAL and create(cd(), None)[0] == EINVAL                                  # 1. null arguments
    assert L.lib.acdsp_ddc_create_polydec(C.byref(cd()), C.byref(pd()), 0, None) == EINVAL
    rc, msg = create(cd(flags=L.FLAG_IN_BYTES, **bad_all), pd(), 6)                                                 # 2. unknown ddc_flags bits
    assert rc == EINVAL and "ddc_flags" in msg
    for c, p in ((cd(flags=L.FLAG_IN_BYTES, **bad_all), pd()), (cd(**bad_all), pd(flags=L.FLAG_IN_BYTES)),         # 3. a byte flag on a stage
                 (cd(**bad_all), pd(flags=L.FLAG_OUT_BYTES)), (cd(flags=L.FLAG_OUT_BYTES, **bad_all), pd())):
        assert create(c, p, L.DDC_IN_BYTES)[0] == EUNSUPPORTED
    rc, msg = create(cd(**bad_all), pd(), L.DDC_IN_BYTES)                                                           # 4. IN_BYTES on 16-bit samples
    assert rc == EINVAL and "1-byte container" in msg
    rc, msg = create(cd(**bad_all), pd())                                                                           # 5. an interpolator
    assert rc == EINVAL and "decimator" in msg
    rc, msg = create(cd(n_channels=5, fout=A.Fmt(40, 21)), pd())                                                    # 6. channel count / device
    assert rc == EINVAL and "same channels" in msg
    rc, msg = create(cd(), pd(device=1, fin=A.Fmt(40, 21)))
    assert rc == EINVAL and "same channels" in msg
    for c, p in ((cd(fout=A.Fmt(40, 21)), pd(n_taps=0)), (cd(), pd(fin=A.Fmt(40, 21), n_taps=0))):                  # 7. not the INT_TYPE
        rc, msg = create(c, p)
        assert rc == EINVAL and "<36,21>" in msg
    assert create(cd(), pd(n_taps=0))[0] == EUNSUPPORTED                                                           # then the stage creates
    assert create(cd(), pd())[0] == 0


# 7. graph capture: whole groups replay and continue the stream, a call that would change the queue length is refused
def test_captured_fused_call_replays_and_partial_groups_are_refused():
    g = CFG5
    rng = np.random.default_rng(46)
    k = 16 * 2 * 700                   # R DF 700 samples, longer than the history: the captured call updates it in place
    x = rng.integers(-32768, 32768, size=(2, 2 * k))
    c = polydec_coeffs(g["n_taps"], g["df"], g["fc"])
    yo = ref(g, FO, A.Fmt(36, 21), c, x)
    ddc = make(g, FO, 2)
    ddc.set_coeffs(c)
    assert ddc.path == "fused"
    xs = torch.from_numpy(x.copy()).to(torch.int16).cuda()
    buf = xs[:, :k].clone()
    odd = torch.zeros((2, k + 16), dtype=torch.int16, device="cuda")
    ddc.run(buf)                       # the plans of window phase 0 go up in an eager call, in front of the capture
    ddc.reset()
    graph, y, msg = refused_under_capture(lambda: ddc.run(buf), lambda: ddc.run(odd))   # n_in = R DF k + R
    assert "R * DF" in msg, msg
    ddc.reset()                        # whatever the capture set-up counted: the stream starts from the constructed state
    torch.cuda.synchronize()
    for i in range(2):                 # two replays on changed input contents continue the stream like two eager calls
        buf.copy_(xs[:, i * k:(i + 1) * k])
        y.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(y.cpu().numpy().astype(np.int64), yo[:, 700 * i:700 * (i + 1)]), "replay %d differs from the eager stream" % i


# 8. fused mode with the decimation phase left mid-period while a word waits: stage A's window phase (first = (R - t_total % R) % R) and stage
# B's queue phase (q = ceil(t_total / R) % DF) move independently
@pytest.mark.parametrize("R", FUSED_RATES)
def test_fused_streaming_across_decimation_phases(R):
    g = dict(CFG5, R=R)
    rng = np.random.default_rng(47 + R)
    # bursts of any length in slot-padded rows: t_total % R takes many values, with q = 0 and q = 1 in front of them; a burst of 3 samples
    # that emits no word, one of R + 1 that emits one or two, a long one over two chunks, a ragged rest
    bursts = [R * 301 + 5, R * 200 + 7, 3, R + 1, R * 1301 + 9, 11, R * 2 * 2 * CHUNK + R * 77 + 13]
    splits = np.cumsum(bursts).tolist()
    x = rng.integers(-32768, 32768, size=(2, splits[-1] + R * 450 + 1))
    c = polydec_coeffs(g["n_taps"], g["df"], g["fc"])
    ddc = make(g, FO, 2)
    ddc.set_coeffs(c)
    assert ddc.path == "fused"
    assert 33 <= ddc.int_type.W <= 40
    counts = []
    y = run_stream(ddc, x, splits, counts, pad=True)
    yo = ref(g, FO, ddc.int_type, c, x, splits)
    assert 0 in counts and y.shape == yo.shape and np.array_equal(y, yo)
    assert ddc.path == "fused"


# 9. graph capture on the two stage kernels, DF 3 with one word waiting at capture time: whole groups replay and continue the stream; a word count
# that is no multiple of DF, and a call the intermediate rows would have to grow for, are refused
def test_captured_two_kernel_call_replays_with_a_word_waiting():
    g = dict(CFG5, n_taps=40, df=3)
    rng = np.random.default_rng(48)
    na, k = 16 * 3001, 16 * 3000       # 3001 words: 1000 outputs and one waits; then 1 + 3000 words per call: 1000 outputs, one waits again
    x = rng.integers(-32768, 32768, size=(2, na + 2 * k))
    c = polydec_coeffs(g["n_taps"], g["df"], g["fc"])
    yo = ref(g, FO, A.Fmt(36, 21), c, x, [na, na + k])
    ddc = make(g, FO, 2)
    ddc.set_coeffs(c)
    assert ddc.path == "two_kernels"
    xs = torch.from_numpy(x.copy()).to(torch.int16).cuda()
    assert np.array_equal(ddc.run(xs[:, :na].contiguous()).cpu().numpy().astype(np.int64), yo[:, :1000])   # eager: plans, rows, the queue
    buf = xs[:, na:na + k].clone()
    odd = torch.zeros((2, 16 * 3001), dtype=torch.int16, device="cuda")
    big = torch.zeros((2, 16 * 6000), dtype=torch.int16, device="cuda")
    _, _, msg = refused_under_capture(lambda: ddc.run(buf), lambda: ddc.run(big))
    assert "intermediate buffer" in msg, msg
    graph, y, msg = refused_under_capture(lambda: ddc.run(buf), lambda: ddc.run(odd))
    assert "multiple of DF" in msg, msg
    torch.cuda.synchronize()
    for i in range(2):                 # the captured calls ran nothing: two replays on changed input contents are the stream's next two calls
        buf.copy_(xs[:, na + i * k:na + (i + 1) * k])
        y.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(y.cpu().numpy().astype(np.int64), yo[:, 1000 * (i + 1):1000 * (i + 2)]), "replay %d differs from the eager stream" % i
