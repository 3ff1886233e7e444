#!/usr/bin/env python3
"""tools/s8_out_shapes.py -- what 1-byte OUTPUT rows (Fir(in_bytes=True, out_bytes=True), ACDSP_FLAG_OUT_BYTES) are worth on the byte-sample FIR
path ("mfma_s8") against the int16 output containers of the same handle.

One process.  Per shape three handles on the same int8 rows of signed <8,2> samples, <16,2> coefficients, ACC <48,28>: two control arms with
ACDSP_FLAG_IN_BYTES only, into <16,I_o,RND,SAT> (the same code run twice, so the spread between two runs of one kernel is on record beside
the ratio), and the doubly flagged handle into <8,I_o,RND,SAT>.  The three arms alternate call by call: WARMUP rounds, then REPS timed rounds;
the times are the handles' own kernel_stats (HIP events around the main kernel).  One JSON line per shape: avg / min ms of the three arms,
ratio = out8 / out16 (avg), spread = |second control / first control - 1|, faster = ratio < 1 - spread, the floor of the ratio by bytes
(2 B against 3 B per sample), the share of 8 TB/s both arms reach, the shader clock measured right behind the last call of each arm, and
whether the outputs equal the CPU oracle (OUT_TYPE of each arm; the first ORACLE_N samples of the first and the last channel, which start
from the zero history both sides share)."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ac_dsp_amd as A  # noqa: E402
from bench import windowed_sinc_raw  # noqa: E402
from oracle import OracleFir, Fmt as OFmt  # noqa: E402

WARMUP, REPS = 3, 20
ORACLE_N = 8192
FIN, FC, FA = A.Fmt(8, 2), A.Fmt(16, 2), A.Fmt(48, 28)
HBM_BYTES_PER_S = 8e12


def dense(n_taps):
    return np.random.default_rng(1).integers(-32768, 32640, size=n_taps, dtype=np.int64)


SHAPES = [
    # name, taps, channels, coefficient set, OUT integer bits (unity-gain sets fill <.,2>; a dense set of N taps needs about log2(sqrt(N)) + 4 more)
    ("15 taps, windowed sinc", 15, 1024, windowed_sinc_raw(15, 0.1, FC.F), 2),
    ("63 taps, windowed sinc", 63, 1024, windowed_sinc_raw(63, 0.1, FC.F), 2),
    ("255 taps, windowed sinc", 255, 1024, windowed_sinc_raw(255, 0.1, FC.F), 2),
    ("1023 taps, windowed sinc", 1023, 1024, windowed_sinc_raw(1023, 0.05, FC.F), 2),
    ("255 taps, dense", 255, 1024, dense(255), 8),
    ("4097 taps, dense", 4097, 64, dense(4097), 10),
]
N = 1 << 20


def o(f):
    return OFmt(f.W, f.I, f.S, f.Q, f.O)


def main():
    only = sys.argv[1] if len(sys.argv) > 1 else None
    for name, taps, n_ch, coeffs, i_o in SHAPES:
        if only and only not in name:
            continue
        fo = {"out16": A.Fmt(16, i_o, True, "RND", "SAT"), "out8": A.Fmt(8, i_o, True, "RND", "SAT")}
        fo["out16_again"] = fo["out16"]
        arms = [("out16", False), ("out8", True), ("out16_again", False)]
        eng = {}
        for arm, flag in arms:
            eng[arm] = A.Fir(taps, "SHIFT_REG", FIN, FC, FA, fo[arm], n_channels=n_ch, kind="load", in_bytes=True, out_bytes=flag)
            eng[arm].set_coeffs(coeffs)
        x16 = torch.empty((n_ch, N), dtype=torch.int16, device="cuda")
        A.fill_stimulus(x16, 0xACD5, 8)
        x8 = x16.to(torch.int8)
        del x16
        ys = {arm: torch.empty((n_ch, N), dtype=eng[arm].out_dtype, device="cuda") for arm, _ in arms}
        # the first call of every handle starts from the zero history: its head is what the oracle sees
        rows = [0, n_ch - 1]
        xo = x8[rows, :ORACLE_N].cpu().numpy().astype(np.int64)
        equal = {}
        for arm, _ in arms:
            eng[arm].run(x8, ys[arm])
            want = OracleFir(taps, "SHIFT_REG", o(FIN), o(FC), o(FA), o(fo[arm]), n_ch=2).run(coeffs, xo)
            equal[arm] = bool(np.array_equal(ys[arm][rows, :ORACLE_N].cpu().numpy().astype(np.int64), want))
        clock = {}
        for r in range(WARMUP + REPS):
            for arm, _ in arms:
                eng[arm].run(x8, ys[arm])
                if r == WARMUP + REPS - 1:
                    clock[arm] = A.diag_shader_clock_mhz(0)
        torch.cuda.synchronize()
        st = {arm: eng[arm].kernel_stats(REPS) for arm, _ in arms}
        ratio = st["out8"][0] / st["out16"][0]
        spread = abs(st["out16_again"][0] / st["out16"][0] - 1.0)
        samples = n_ch * N
        row = {
            "shape": name, "n_taps": taps, "channels": n_ch, "samples": N, "out16": "<16,%d,RND,SAT>" % i_o, "out8": "<8,%d,RND,SAT>" % i_o,
            "path_out16": eng["out16"].path, "path_out8": eng["out8"].path,
            "ms_out16_avg": round(st["out16"][0], 4), "ms_out16_min": round(st["out16"][1], 4),
            "ms_out8_avg": round(st["out8"][0], 4), "ms_out8_min": round(st["out8"][1], 4),
            "ms_out16_again_avg": round(st["out16_again"][0], 4), "ms_out16_again_min": round(st["out16_again"][1], 4),
            "ratio_out8_over_out16": round(ratio, 4), "spread_out16": round(spread, 4), "faster": bool(ratio < 1.0 - spread),
            "floor_by_bytes": round(2.0 / 3.0, 4),
            "mfma_issued_out16": eng["out16"].mfma_issued(), "mfma_issued_out8": eng["out8"].mfma_issued(),
            "bytes_per_sample_out16": 3, "bytes_per_sample_out8": 2,
            "share_of_8TBps_out16": round(3.0 * samples / (st["out16"][0] * 1e-3) / HBM_BYTES_PER_S, 4),
            "share_of_8TBps_out8": round(2.0 * samples / (st["out8"][0] * 1e-3) / HBM_BYTES_PER_S, 4),
            "clock_mhz_out16": round(clock["out16"], 1), "clock_mhz_out8": round(clock["out8"], 1), "clock_mhz_out16_again": round(clock["out16_again"], 1),
            "equal_to_oracle_out16": equal["out16"], "equal_to_oracle_out8": equal["out8"], "equal_to_oracle_out16_again": equal["out16_again"],
            "oracle_slice": "channels 0 and %d, first %d samples" % (n_ch - 1, ORACLE_N),
            "timed_calls_per_arm": REPS, "warmup_calls_per_arm": WARMUP,
        }
        print(json.dumps(row), flush=True)
        del eng, x8, ys
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
