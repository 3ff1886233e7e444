#!/usr/bin/env python3
"""tools/s8_shapes.py -- what the byte-sample FIR path (Fir(in_bytes=True), "mfma_s8") is worth against the int16 containers of the same values.

One process.  Per shape three handles on the same signed <8,2> samples, <16,2> coefficients and <16,.,RND,SAT> output: the flagged one on int8
rows, and two unflagged ones on int16 rows (the path an 8-bit stream takes without the flag: "mfma_i8" up to 1025 taps, "mfma_long" above) --
the second of them is the same code run again, so the spread between two runs of one kernel is on record beside the ratio.  The three arms
alternate call by call: WARMUP rounds, then REPS timed rounds; the times are the handles' own kernel_stats (HIP events around the main kernel).
One JSON line per shape: avg / min ms of the three arms, ratio = s8 / int16 (avg), spread = |int16 second run / int16 - 1|, mfma_issued and
algorithmic bytes per sample of both, the shader clock measured right behind the last call of each arm, and whether the outputs are equal."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ac_dsp_amd as A  # noqa: E402
from bench import windowed_sinc_raw  # noqa: E402

WARMUP, REPS = 3, 20
FIN, FC, FA = A.Fmt(8, 2), A.Fmt(16, 2), A.Fmt(48, 28)


def dense(n_taps):
    return np.random.default_rng(1).integers(-32768, 32640, size=n_taps, dtype=np.int64)


SHAPES = [
    # name, taps, channels, coefficient set, OUT integer bits (unity-gain sets fill <16,2>; a dense set of N taps needs about log2(sqrt(N)) + 4 more)
    ("63 taps, windowed sinc", 63, 1024, windowed_sinc_raw(63, 0.1, FC.F), 2),
    ("255 taps, windowed sinc", 255, 1024, windowed_sinc_raw(255, 0.1, FC.F), 2),
    ("1023 taps, windowed sinc", 1023, 1024, windowed_sinc_raw(1023, 0.05, FC.F), 2),
    ("255 taps, dense", 255, 1024, dense(255), 8),
    ("4097 taps, dense", 4097, 64, dense(4097), 10),
    ("16384 taps, dense", 16384, 64, dense(16384), 11),
]
N = 1 << 20


def main():
    only = sys.argv[1] if len(sys.argv) > 1 else None
    for name, taps, n_ch, coeffs, i_o in SHAPES:
        if only and only not in name:
            continue
        fo = A.Fmt(16, i_o, True, "RND", "SAT")
        arms = [("i16", False), ("s8", True), ("i16_again", False)]
        eng = {}
        for arm, flag in arms:
            eng[arm] = A.Fir(taps, "SHIFT_REG", FIN, FC, FA, fo, n_channels=n_ch, kind="load", in_bytes=flag)
            eng[arm].set_coeffs(coeffs)
        x16 = torch.empty((n_ch, N), dtype=torch.int16, device="cuda")
        A.fill_stimulus(x16, 0xACD5, 8)
        x8 = x16.to(torch.int8)
        xs = {"i16": x16, "s8": x8, "i16_again": x16}
        ys = {arm: torch.empty((n_ch, N), dtype=torch.int16, device="cuda") for arm, _ in arms}
        clock = {}
        for r in range(WARMUP + REPS):
            for arm, _ in arms:
                eng[arm].run(xs[arm], ys[arm])
                if r == WARMUP + REPS - 1:
                    clock[arm] = A.diag_shader_clock_mhz(0)
        torch.cuda.synchronize()
        st = {arm: eng[arm].kernel_stats(REPS) for arm, _ in arms}
        row = {
            "shape": name, "n_taps": taps, "channels": n_ch, "samples": N, "out": "<16,%d,RND,SAT>" % i_o,
            "path_i16": eng["i16"].path, "path_s8": eng["s8"].path,
            "ms_i16_avg": round(st["i16"][0], 4), "ms_i16_min": round(st["i16"][1], 4),
            "ms_s8_avg": round(st["s8"][0], 4), "ms_s8_min": round(st["s8"][1], 4),
            "ms_i16_again_avg": round(st["i16_again"][0], 4), "ms_i16_again_min": round(st["i16_again"][1], 4),
            "ratio_s8_over_i16": round(st["s8"][0] / st["i16"][0], 4),
            "spread_i16": round(abs(st["i16_again"][0] / st["i16"][0] - 1.0), 4),
            "mfma_issued_i16": eng["i16"].mfma_issued(), "mfma_issued_s8": eng["s8"].mfma_issued(),
            "bytes_per_sample_i16": 4, "bytes_per_sample_s8": 3,
            "clock_mhz_i16": round(clock["i16"], 1), "clock_mhz_s8": round(clock["s8"], 1), "clock_mhz_i16_again": round(clock["i16_again"], 1),
            "outputs_equal": bool(torch.equal(ys["i16"], ys["s8"])),
            "timed_calls_per_arm": REPS, "warmup_calls_per_arm": WARMUP,
        }
        print(json.dumps(row), flush=True)
        del eng, x16, x8, xs, ys
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
