#!/usr/bin/env python3
"""tools/intr_shapes.py -- the interpolating kernels outside the two bench rows, 1024 channels.  One line per shape: ms per call (events on
the current stream) and TB/s of read + written bytes.  A/B two builds by running it once per build (ACDSP_LIB=..., or PYTHONPATH of the other
tree), alternating.

  (no argument)   fir_up_kernel: ac_cic_intr_full at R = 4 / 8 / 16 on 16- and 32-bit inputs
  long [NxIF ...] [--inputs N] [--channels C] [--calls K] [--fir]
                  ac_poly_intr with 65 taps per phase and more (polyintr_long.hip on this build; the tiled int64 kernel on a build without
                  it, which refuses more than 2048 taps): by default 64x4 129x8 480x2 2048x8 8192x2 16383x1 on 2^20 inputs.  --fir: beside
                  each row, IF separate Fir calls of nt taps (the same products without the merge; nt >= 1026 only)"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

import ac_dsp_amd as A  # noqa: E402


def long_rows(argv):
    import argparse
    import numpy as np
    ap = argparse.ArgumentParser(prog="intr_shapes.py long")
    ap.add_argument("shapes", nargs="*", default=["64x4", "129x8", "480x2", "2048x8", "8192x2", "16383x1"], help="NTAPSxIF")
    ap.add_argument("--inputs", type=int, default=1 << 20)
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--fir", action="store_true")
    args = ap.parse_args(argv)
    shapes = [tuple(int(v) for v in a.split("x")) for a in args.shapes]
    n, n_ch, K, fir = args.inputs, args.channels, args.calls, args.fir
    fin = fc = A.Fmt(16, 2)
    fa, fo = A.Fmt(48, 20), A.Fmt(16, 10, True, "RND", "SAT")

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        call()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(K):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / K

    x = torch.empty((n_ch, n), dtype=torch.int16, device="cuda")
    A.fill_stimulus(x, 1, 16)
    for nt_, ifac in shapes:
        ft = "FOLD_EVEN" if nt_ % 2 == 0 else "FOLD_ODD"      # the symmetric prototypes of a synthesis bank, phases paired
        csz = ((nt_ // 2 - 1) + (ifac - 1) * nt_ // 2 if ft == "FOLD_EVEN" else (nt_ - 1) // 2 + (nt_ // 2 + 1) * (ifac - 1)) + 1
        rng = np.random.default_rng(nt_ + ifac)
        c = rng.integers(-16000, 16000, size=csz, dtype=np.int64)
        try:
            eng = A.PolyIntr(nt_, csz, ifac, ft, fin, fc, fa, fo, n_channels=n_ch)
        except A.AcdspError as e:
            print("poly_intr %5d x %-3d %s: refused by this build (%s)" % (nt_, ifac, ft, str(e)[:60]))
            continue
        eng.set_ctrl(c, np.ones(ifac, dtype=np.int64), ifac - 1 - np.arange(ifac))
        y = torch.empty((n_ch, n * ifac), dtype=torch.int16, device="cuda")
        try:
            eng.run(x[:, :4096], out=y)                       # the stream's first call: later calls carry the head launch
            call = lambda: eng.run(x, out=y)                  # noqa: E731
        except TypeError:                                     # (a build whose run() allocates its output)
            eng.run(x[:, :4096])
            call = lambda: eng.run(x)                         # noqa: E731
        ms = timed(call)
        gb = (x.numel() + n_ch * n * ifac) * 2 / 1e9
        line = "poly_intr %5d x %-3d %s %d ch x %d: %9.3f ms  %.2f TB/s  path %s" % (nt_, ifac, ft, n_ch, n, ms, gb / ms, eng.path)
        if hasattr(eng, "long_geometry"):
            line += "  slab/group/bytes %s" % (eng.long_geometry(),)
        del eng, y
        if fir and nt_ + 1 >= 1026:
            f = A.Fir(nt_ + 1, "SHIFT_REG", fin, fc, fa, fo, n_channels=n_ch)
            f.set_coeffs(rng.integers(-32768, 32640, size=nt_ + 1, dtype=np.int64))
            yf = torch.empty((n_ch, n), dtype=torch.int16, device="cuda")
            line += "  | %d x Fir(%d taps, %s): %.3f ms" % (ifac, nt_ + 1, f.path, ifac * timed(lambda: f.run(x, yf)))
            del f, yf
        print(line, flush=True)


if len(sys.argv) > 1 and sys.argv[1] == "long":
    long_rows(sys.argv[2:])
    sys.exit(0)

n_ch = 1024
K = 10
M_OF = {7: 2}
for w_in, R, n in ((32, 4, 1 << 19), (32, 8, 1 << 18), (32, 16, 1 << 17), (16, 4, 1 << 19), (16, 8, 1 << 18), (16, 16, 1 << 17), (32, 7, 1 << 18), (16, 7, 1 << 18), (32, 3, 1 << 19), (32, 5, 1 << 18), (16, 6, 1 << 18)):
    fin = A.Fmt(w_in, w_in // 2)
    N = 5 if w_in == 32 or R < 16 else 4
    M = M_OF.get(R, 1)
    probe = A.Cic(True, R, M, N, fin, fin, n_channels=1)
    it = probe.int_type
    fout = A.Fmt(it.W, it.I)
    eng = A.Cic(True, R, M, N, fin, fout, n_channels=n_ch)
    x = torch.empty((n_ch, n), dtype=A.torch_dtype_for(fin), device="cuda")
    A.fill_stimulus(x, 1, w_in)
    y = torch.empty((n_ch, n * R + 64), dtype=A.torch_dtype_for(fout), device="cuda")
    for _ in range(3):
        eng.reset()
        out = eng.run(x, y)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(K):
        out = eng.run(x, y)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / K
    gb = (x.numel() * x.element_size() + out.numel() * out.element_size()) / 1e9
    print("cic_intr N%d M%d R%-2d <%d> -> <%d,%d> (%d-byte outputs): %.3f ms  %.2f TB/s  path %s" % (N, M, R, w_in, it.W, it.I, out.element_size(), ms, gb / ms, eng.path))
    del eng, x, y, out
