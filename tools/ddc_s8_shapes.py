#!/usr/bin/env python3
"""tools/ddc_s8_shapes.py -- what byte rows (Ddc(in_bytes=True), ACDSP_DDC_IN_BYTES) are worth to the DDC cascade against int16 rows of the
same values.

One process.  Per shape three handles on the same raw 8-bit words: the byte handle on int8 / uint8 rows, and two unflagged handles on int16
rows -- the second of them is the same code run again, so the spread between two runs of one kernel is on record beside the ratio.  The
int16 arm is the cascade an 8-bit stream takes today after widening, on its best kernel: the words stand in <16,1> containers (the
bench.py `ddc` types: INT_TYPE <36,21>, <16,1> coefficients, <60,30> sums), and the byte arm's IN / ACC / OUT types carry eight fraction bits
fewer (<8,1>: <60,38> sums) so that both arms shift, round and saturate the same raw sums: the raw outputs are equal word for word, which
every row asserts.  The three arms alternate call by call: WARMUP rounds, then REPS timed rounds.  ms per call are torch stream events around
the whole run() -- the history update behind the cascade kernel counts (kernel_stats does not see it).  Every call starts its handle from
reset(), so that each timed call is the same whole-row call at decimation phase 0.
One JSON line per shape: avg / min ms of the three arms, ratio = s8 / int16 (avg), spread = |int16 second run / int16 - 1|, faster = ratio <
1 - spread, the paths, the algorithmic bytes per input sample of both arms (in_eb + out_eb / R) with the GB/s they amount to and their share
of 8 TB/s, and whether the outputs are equal."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

import ac_dsp_amd as A  # noqa: E402
from bench import windowed_sinc_raw  # noqa: E402  (the benchmark's 127-tap low-pass)

WARMUP, REPS = 3, 20
HBM_GBS = 8000.0
FC = A.Fmt(16, 1)
N_TAPS = 127


# name, channels, samples, R, N, signed samples, OUT_TYPE of the int16 arm (W, I, Q, O); the byte arm's OUT_TYPE has the same width and eight
# (unsigned: fifteen) integer bits more
SHAPES = [
    ("bench.py ddc geometry", 4096, 1 << 20, 16, 5, True, (24, 9, "RND", "SAT")),
    ("512 streams", 512, 1 << 20, 16, 5, True, (24, 9, "RND", "SAT")),
    ("<8,8,false> on uint8 rows", 4096, 1 << 20, 16, 5, False, (24, 9, "RND", "SAT")),
    ("32-bit OUT (64-bit epilogue)", 4096, 1 << 20, 16, 5, True, (32, 12, "RND", "WRAP")),
    ("R 64 N 4 (two kernels on both arms)", 1024, 1 << 20, 64, 4, True, (24, 9, "RND", "SAT")),
]


def main():
    only = sys.argv[1] if len(sys.argv) > 1 else None
    c = windowed_sinc_raw(N_TAPS, 0.2, FC.F)
    for name, n_ch, n, R, N, signed, (ow, oi, oq, oo) in SHAPES:
        if only and only not in name:
            continue
        fin8 = A.Fmt(8, 1) if signed else A.Fmt(8, 8, False)
        dfrac = 15 - fin8.F                                    # fraction bits the <16,1> container has over the 8-bit type
        fin16, fa16, fo16 = A.Fmt(16, 1), A.Fmt(60, 30), A.Fmt(ow, oi, True, oq, oo)
        fa8, fo8 = A.Fmt(60, 30 + dfrac), A.Fmt(ow, oi + dfrac, True, oq, oo)
        arms = ["i16", "s8", "i16_again"]
        eng = {
            "i16": A.Ddc(R, 1, N, fin16, N_TAPS, "SHIFT_REG", FC, fa16, fo16, n_channels=n_ch),
            "s8": A.Ddc(R, 1, N, fin8, N_TAPS, "SHIFT_REG", FC, fa8, fo8, n_channels=n_ch, in_bytes=True),
            "i16_again": A.Ddc(R, 1, N, fin16, N_TAPS, "SHIFT_REG", FC, fa16, fo16, n_channels=n_ch),
        }
        for e in eng.values():
            e.set_coeffs(c)
        x16 = torch.empty((n_ch, n), dtype=torch.int16, device="cuda")
        A.fill_stimulus(x16, 0xACD5, 8)                        # signed 8-bit words
        if not signed:
            x16 += 128                                         # the same ADC in offset binary: 0 .. 255
        x8 = x16.to(eng["s8"].in_dtype)
        xs = {"i16": x16, "s8": x8, "i16_again": x16}
        no = eng["i16"].out_count(n)
        ys = {arm: torch.empty((n_ch, (no + 7) // 8 * 8), dtype=torch.int32, device="cuda") for arm in arms}
        ev = {arm: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)] for arm in arms}
        for r in range(WARMUP + REPS):
            for arm in arms:
                eng[arm].reset()
                if r >= WARMUP:
                    ev[arm][r - WARMUP][0].record()
                eng[arm].run(xs[arm], ys[arm])
                if r >= WARMUP:
                    ev[arm][r - WARMUP][1].record()
        torch.cuda.synchronize()
        ms = {arm: [a.elapsed_time(b) for a, b in ev[arm]] for arm in arms}
        avg = {arm: sum(ms[arm]) / REPS for arm in arms}
        out_eb = 4
        bps = {"i16": 2 + out_eb / R, "s8": 1 + out_eb / R}

        def gbs(arm, key):
            return bps[key] * n_ch * n / (avg[arm] * 1e-3) / 1e9

        equal = bool(torch.equal(ys["i16"][:, :no], ys["s8"][:, :no]))
        ratio, spread = avg["s8"] / avg["i16"], abs(avg["i16_again"] / avg["i16"] - 1.0)
        row = {
            "shape": name, "channels": n_ch, "samples": n, "R": R, "N": N, "taps": N_TAPS, "in_s8": repr(fin8), "out_i16": repr(fo16), "out_s8": repr(fo8),
            "int_type_i16": repr(eng["i16"].int_type), "int_type_s8": repr(eng["s8"].int_type),
            "path_i16": eng["i16"].path, "path_s8": eng["s8"].path,
            "ms_i16_avg": round(avg["i16"], 4), "ms_i16_min": round(min(ms["i16"]), 4),
            "ms_s8_avg": round(avg["s8"], 4), "ms_s8_min": round(min(ms["s8"]), 4),
            "ms_i16_again_avg": round(avg["i16_again"], 4), "ms_i16_again_min": round(min(ms["i16_again"]), 4),
            "kernel_ms_i16": round(eng["i16"].kernel_stats(REPS)[0], 4), "kernel_ms_s8": round(eng["s8"].kernel_stats(REPS)[0], 4),
            "ratio_s8_over_i16": round(ratio, 4), "spread_i16": round(spread, 4), "faster": bool(ratio < 1.0 - spread),
            "expected_by_bytes": round(bps["s8"] / bps["i16"], 4),
            "bytes_per_sample_i16": round(bps["i16"], 4), "bytes_per_sample_s8": round(bps["s8"], 4),
            "gbs_i16": round(gbs("i16", "i16"), 1), "gbs_s8": round(gbs("s8", "s8"), 1),
            "hbm_share_i16": round(gbs("i16", "i16") / HBM_GBS, 3), "hbm_share_s8": round(gbs("s8", "s8") / HBM_GBS, 3),
            "outputs_equal": equal, "timed_calls_per_arm": REPS, "warmup_calls_per_arm": WARMUP,
        }
        print(json.dumps(row), flush=True)
        assert equal, "the byte arm and the int16 arm disagree on " + name
        del eng, x16, x8, xs, ys
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
