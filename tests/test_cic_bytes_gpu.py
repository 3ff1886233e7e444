"""GPU parity tests of ac_cic_dec_full on byte samples (ACDSP_FLAG_IN_BYTES, Cic(in_bytes=True)): an IN_TYPE of up to 8 bits in 1-byte
containers.  Stage 1 of the two-stage kernel runs on ONE sample plane (cic2_kernels.hpp, shapes s8_r16 / s8_r8 / s8_r4), everything else on
the recurrence kernel's 1-byte instantiation (cic.hip).  Bit-exact against the CPU oracle (reference include/ac_dsp/ac_cic_full_core.h:80-135,
228-255, ac_cic_dec_full.h:187-222), through the C ABI."""
import struct

import numpy as np
import pytest
import torch

import ac_dsp_amd as A
from oracle import OracleCic
from helpers import ofmt
from test_cic2_gpu import rand_raw, oracle_calls
from test_graph_gpu import _capture_and_check

pytestmark = pytest.mark.gpu


def fmt_of(W, I, s):
    return A.Fmt(W, I, s == "s")


def int_fmt(R, M, N, fin):
    it = A.Cic(False, R, M, N, fin, fin, in_bytes=True).int_type
    return A.Fmt(it.W, it.I)


def to_rows(seg, dt):
    return torch.from_numpy(np.ascontiguousarray(seg)).to(dt)


def run_calls(cic, x, lengths):
    """The stream x in calls of the given lengths, each from its own 16-byte aligned buffer of the handle's input containers whose row stride is
    ceil(len / 16) * 16 + 16 samples, so that calls of ANY length -- every decimation phase -- meet the row rule of the matrix-core kernel."""
    dt = cic.in_dtype
    outs, paths, pos = [], [], 0
    for ln in lengths:
        buf = torch.zeros((x.shape[0], (ln + 15) // 16 * 16 + 16), dtype=dt, device="cuda")
        assert buf.data_ptr() % 16 == 0
        buf[:, :ln] = to_rows(x[:, pos:pos + ln], dt).cuda()
        pos += ln
        outs.append(cic.run(buf[:, :ln]).cpu().numpy().astype(np.int64))
        paths.append(cic.path)
    assert pos == x.shape[1]
    return np.concatenate(outs, axis=1), paths


def same(y, yo, what=""):
    assert y.shape == yo.shape, (what, y.shape, yo.shape)
    bad = np.argwhere(y != yo)
    assert bad.size == 0, "%s: %d mismatches, first at %s: got %d want %d" % (what, len(bad), bad[0], y[tuple(bad[0])], yo[tuple(bad[0])])


def full_scale_stream(rng, fin, n_ch, n):
    x = rand_raw(rng, fin, (n_ch, n))
    x[1, :20000] = (1 << (fin.W - 1)) - 1 if fin.S else (1 << fin.W) - 1      # full-scale runs: the integrators wrap many times over
    x[2, 5000:60000] = -(1 << (fin.W - 1)) if fin.S else 0
    return x


# 1. ragged calls through every decimation phase, every compiled byte shape
TWO_STAGE = [
    # W, I, S, R, M, N, (R1, R2)
    (8, 1, "s", 32, 1, 4, (16, 2)), (8, 1, "s", 64, 1, 3, (16, 4)), (8, 1, "s", 256, 1, 3, (16, 16)), (8, 1, "s", 128, 2, 3, (16, 8)),
    (8, 1, "s", 32, 1, 6, (16, 2)),        # third digit plane
    (6, 2, "s", 48, 2, 3, (16, 3)),        # a narrow type in a byte
    (8, 1, "s", 24, 1, 4, (8, 3)), (8, 1, "s", 40, 1, 5, (8, 5)), (8, 1, "s", 200, 2, 3, (8, 25)),
    (8, 1, "s", 8, 1, 2, (4, 2)),          # 14-bit INT_TYPE: 2-byte outputs
    (8, 1, "s", 12, 2, 5, (4, 3)), (8, 1, "s", 20, 1, 1, (4, 5)),
    (8, 1, "s", 244, 2, 3, (4, 61)),       # the one case with two warm-up steps
    (8, 8, "u", 64, 1, 4, (16, 4)), (7, 7, "u", 96, 1, 3, (16, 6)), (1, 1, "u", 64, 1, 3, (16, 4)),
]


@pytest.mark.parametrize("W,I,S,R,M,N,rates", TWO_STAGE)
def test_two_stage_byte_decimator_vs_oracle_ragged_calls(W, I, S, R, M, N, rates):
    fin = fmt_of(W, I, S)
    fout = int_fmt(R, M, N, fin)
    rng = np.random.default_rng(W * 1000 + R * 10 + N)
    lengths = [70001, 3, 41003, R - 1, 36864 + 17, 5 * 4096, 1, 30011]
    x = full_scale_stream(rng, fin, 3, sum(lengths))
    cic = A.Cic(False, R, M, N, fin, fout, n_channels=3, in_bytes=True)
    assert cic.two_stage_rates == rates
    assert cic.in_dtype == (torch.int8 if fin.S else torch.uint8)
    y, paths = run_calls(cic, x, lengths)
    same(y, oracle_calls(R, M, N, fin, fout, x, lengths))
    assert paths[0] == "two_stage" and paths[2] == "two_stage", paths


# 2. the recurrence kernel's 1-byte instantiation
@pytest.mark.parametrize("W,I,S,R,M,N", [(8, 1, "s", 37, 1, 3), (8, 1, "s", 6, 1, 3), (8, 1, "s", 2, 1, 4), (8, 1, "s", 4, 1, 5), (8, 8, "u", 5, 2, 3)])
def test_rates_no_byte_shape_divides_run_the_recurrence_kernel(W, I, S, R, M, N):
    fin = fmt_of(W, I, S)
    fout = int_fmt(R, M, N, fin)
    lengths = [40000, 3, 20001]
    x = full_scale_stream(np.random.default_rng(R), fin, 3, sum(lengths))
    cic = A.Cic(False, R, M, N, fin, fout, n_channels=3, in_bytes=True)
    assert cic.two_stage_rates == (0, 0)
    y, paths = run_calls(cic, x, lengths)
    assert paths == ["recurrence"] * 3, paths
    same(y, oracle_calls(R, M, N, fin, fout, x, lengths))


def test_rows_one_byte_off_alignment_run_the_recurrence_kernel():
    fin, R, M, N = A.Fmt(8, 1), 64, 1, 4
    fout = int_fmt(R, M, N, fin)
    lengths = [40000, 20001]
    n_ch = 3
    x = rand_raw(np.random.default_rng(3), fin, (n_ch, sum(lengths)))
    cic = A.Cic(False, R, M, N, fin, fout, n_channels=n_ch, in_bytes=True)
    assert cic.two_stage_rates == (16, 4)
    outs, pos = [], 0
    for ln in lengths:
        stride = (ln + 15) // 16 * 16 + 16
        flat = torch.zeros(n_ch * stride + 16, dtype=torch.int8, device="cuda")
        rows = flat[1:1 + n_ch * stride].view(n_ch, stride)[:, :ln]
        assert rows.data_ptr() % 16 == 1
        rows.copy_(to_rows(x[:, pos:pos + ln], torch.int8).cuda())
        pos += ln
        outs.append(cic.run(rows).cpu().numpy().astype(np.int64))
        assert cic.path == "recurrence"
    same(np.concatenate(outs, axis=1), oracle_calls(R, M, N, fin, fout, x, lengths))


def test_calls_too_short_for_a_chunk_run_the_recurrence_kernel():
    fin, R, M, N = A.Fmt(8, 1), 64, 1, 4
    fout = int_fmt(R, M, N, fin)
    lengths = [1, R - 1, R, R + 1] * 3
    x = rand_raw(np.random.default_rng(4), fin, (1, sum(lengths)))
    cic = A.Cic(False, R, M, N, fin, fout, n_channels=1, in_bytes=True)
    y, paths = run_calls(cic, x, lengths)
    assert set(paths) == {"recurrence"}, paths
    same(y, oracle_calls(R, M, N, fin, fout, x, lengths))


# 3. both kernels and the state blob
def test_both_kernels_agree_and_share_state_blobs_clone_and_reset():
    fin, R, M, N, n_ch = A.Fmt(8, 1), 64, 2, 3, 4
    fout = int_fmt(R, M, N, fin)
    lengths = [45001, 52003]
    x = rand_raw(np.random.default_rng(7), fin, (n_ch, sum(lengths)))

    def mk(**kw):
        kw.setdefault("in_bytes", True)
        return A.Cic(False, R, M, N, fin, fout, n_channels=n_ch, **kw)

    new, old = mk(), mk(force_generic=True)
    y_new, p_new = run_calls(new, x, lengths)
    y_old, p_old = run_calls(old, x, lengths)
    assert p_new[0] == "two_stage" and p_old == ["recurrence", "recurrence"]
    yo = oracle_calls(R, M, N, fin, fout, x, lengths)
    same(y_new, y_old, "two-stage against force_generic")
    same(y_new, yo, "two-stage against the oracle")
    # first call on one handle, blob into the other kind of handle, second call there
    for a_kw, b_kw in (({}, {"force_generic": True}), ({"force_generic": True}, {})):
        a, b = mk(**a_kw), mk(**b_kw)
        y0, _ = run_calls(a, x[:, :lengths[0]], lengths[:1])
        blob = a.state()
        assert struct.unpack_from("<I", blob, 20)[0] == 1, "elem_bytes of the state header"
        assert len(blob) != len(b.state())
        b.set_state(blob)
        y1, _ = run_calls(b, x[:, lengths[0]:], lengths[1:])
        same(np.concatenate([y0, y1], axis=1), yo, str((a_kw, b_kw)))
    # blobs of an unflagged handle of the same descriptor are refused, and the other way round
    flagged, twin16 = mk(), mk(in_bytes=False)
    y0, _ = run_calls(flagged, x[:, :lengths[0]], lengths[:1])
    run_calls(twin16, x[:, :lengths[0]], lengths[:1])
    for dst, src in ((flagged, twin16), (twin16, flagged)):
        with pytest.raises(A.AcdspError) as e:
            dst.set_state(src.state())
        assert e.value.code == 1, e.value                     # ACDSP_EINVAL
    # clone() mid-stream: both continue the stream on their own
    cl = flagged.clone()
    assert cl.in_dtype == torch.int8 and cl.in_bytes
    for h, what in ((flagged, "after the refused blob"), (cl, "clone")):
        y1, p1 = run_calls(h, x[:, lengths[0]:], lengths[1:])
        same(np.concatenate([y0, y1], axis=1), yo, what)
        assert p1 == ["two_stage"]
    # reset(): the stream starts again
    flagged.reset()
    y_again, _ = run_calls(flagged, x, lengths)
    same(y_again, yo, "after reset()")


# 4. OUT_TYPE conversion on the byte path
@pytest.mark.parametrize("q,o,wo,io", [("RND", "SAT", 12, 4), ("RND", "SAT", 20, 4), ("TRN", "WRAP", 18, 2), ("RND_CONV", "SAT_SYM", 24, 12),
                                       ("TRN_ZERO", "SAT_ZERO", 40, 40)])
def test_output_type_conversion_on_the_byte_path(q, o, wo, io):
    fin, R, M, N = A.Fmt(8, 1), 64, 1, 4
    fout = A.Fmt(wo, io, True, q, o)
    lengths = [50000, 33333]
    x = rand_raw(np.random.default_rng(wo), fin, (2, sum(lengths)))
    cic = A.Cic(False, R, M, N, fin, fout, n_channels=2, in_bytes=True)
    y, paths = run_calls(cic, x, lengths)
    assert paths == ["two_stage", "two_stage"]
    same(y, oracle_calls(R, M, N, fin, fout, x, lengths))


# 5. a bank wider than a wave row, rows of whole chunks
def test_many_channels_whole_chunks():
    fin, R, M, N = A.Fmt(8, 1), 32, 1, 5
    fout = int_fmt(R, M, N, fin)
    n_ch, n = 130, 1 << 16
    x = rand_raw(np.random.default_rng(99), fin, (n_ch, n))
    cic = A.Cic(False, R, M, N, fin, fout, n_channels=n_ch, in_bytes=True)
    y, paths = run_calls(cic, x, [n])
    assert paths == ["two_stage"]
    same(y, oracle_calls(R, M, N, fin, fout, x, [n]))


# 6. other entry points
def test_run_host_equals_run():
    fin, R, M, N, n_ch = A.Fmt(8, 1), 64, 1, 4, 3
    fout = int_fmt(R, M, N, fin)
    lengths = [40000, 777, 20001]
    x = rand_raw(np.random.default_rng(11), fin, (n_ch, sum(lengths)))
    dev = A.Cic(False, R, M, N, fin, fout, n_channels=n_ch, in_bytes=True)
    host = A.Cic(False, R, M, N, fin, fout, n_channels=n_ch, in_bytes=True)
    y, _ = run_calls(dev, x, lengths)
    outs, pos = [], 0
    for ln in lengths:
        outs.append(host.run_host(x[:, pos:pos + ln]).astype(np.int64))
        pos += ln
    same(np.concatenate(outs, axis=1), y, "run_host against run")
    same(y, oracle_calls(R, M, N, fin, fout, x, lengths), "run against the oracle")


def test_node_layer_shards_byte_rows():
    fin, R, M, N, n_ch = A.Fmt(8, 1), 64, 1, 4, 7
    fout = int_fmt(R, M, N, fin)
    node = A.NodeCic(False, R, M, N, fin, fout, n_ch, [0, 0, 0], in_bytes=True)
    assert node.slices == [(0, 3), (3, 5), (5, 7)]
    orc = OracleCic(False, R, M, N, ofmt(fin), ofmt(fout), n_ch=n_ch)
    rng = np.random.default_rng(22)
    for n in (40000, 1300, 32768):
        x = rand_raw(rng, fin, (n_ch, n))
        xs = []
        for lo, hi in node.slices:
            buf = torch.zeros((hi - lo, (n + 15) // 16 * 16 + 16), dtype=torch.int8, device="cuda")
            buf[:, :n] = to_rows(x[lo:hi], torch.int8).cuda()
            xs.append(buf[:, :n])
        ys = node.run(xs)
        torch.cuda.synchronize()
        same(np.concatenate([y.cpu().numpy().astype(np.int64) for y in ys]), orc.run(x), "node call of %d samples" % n)
    node.close()


# 7. graph capture
def test_byte_decimator_calls_replayed_from_a_graph_continue_the_stream():
    fin, R, M, N = A.Fmt(8, 1), 64, 1, 4
    fout = int_fmt(R, M, N, fin)
    assert fout.W == 32
    nch, cs, nk = 16, 65536, 3

    def make():
        return A.Cic(False, R, M, N, fin, fout, n_channels=nch, in_bytes=True)

    x = torch.from_numpy(np.random.default_rng(24).integers(-128, 128, size=(nk, nch, cs), dtype=np.int8)).cuda()
    eager = make()
    y0 = eager.run(x[0]).cpu().numpy().astype(np.int64)       # one eager call of the same shape first, against the oracle
    assert eager.path == "two_stage"
    same(y0, OracleCic(False, R, M, N, ofmt(fin), ofmt(fout), n_ch=nch).run(x[0].cpu().numpy().astype(np.int64)), "eager call")
    _capture_and_check(make, x, (nch, cs // R), torch.int32)
