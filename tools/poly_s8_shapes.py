#!/usr/bin/env python3
"""tools/poly_s8_shapes.py -- what byte rows (PolyDec(in_bytes=True)) are worth to ac_poly_dec against int16 containers of the same values.

One process.  Per shape three handles on the same signed <8,2> samples and the same coefficient set: the flagged one on int8 rows, and two
unflagged ones on int16 rows (the path an 8-bit stream takes without the flag) -- the second of them is the same code run again, so the
spread between two runs of one kernel is on record beside the ratio.  The three arms alternate call by call: WARMUP rounds, then REPS
timed rounds, each call between two events on the stream (the whole call: main kernel(s) and the history kernel).
One JSON line per shape: avg / min ms of the three arms, ratio = s8 / int16 (avg), spread = |int16 second run / int16 - 1|, the expectation
by arithmetic for an HBM-bound row (1 + oeb / DF) / (2 + oeb / DF), path and ring-shape id of both arms, the algorithmic bytes per input
sample of both and the GB/s they amount to, and whether the outputs are equal."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

import ac_dsp_amd as A  # noqa: E402

WARMUP, REPS = 3, 20
FIN, FC, FA = A.Fmt(8, 2), A.Fmt(16, 2), A.Fmt(40, 20)
FO2, FO8 = A.Fmt(16, 10, True, "RND", "SAT"), A.Fmt(40, 20)
HBM_GBS = 8000.0

SHAPES = [
    # name, channels, samples, NTAPS, DF, OUT_TYPE
    ("bench shape 16 x 8 -> int16", 1024, 1 << 22, 16, 8, FO2),
    ("16 x 8 -> int64", 1024, 1 << 21, 16, 8, FO8),
    ("16 x 2 -> int16", 1024, 1 << 21, 16, 2, FO2),
    ("16 x 2 -> int64", 1024, 1 << 20, 16, 2, FO8),
    ("16 x 4 -> int16", 1024, 1 << 21, 16, 4, FO2),
    ("16 x 4 -> int64", 1024, 1 << 20, 16, 4, FO8),
    ("16 x 16 -> int16", 1024, 1 << 22, 16, 16, FO2),
    ("16 x 16 -> int64", 1024, 1 << 21, 16, 16, FO8),
    ("16 x 3 -> int16 (window-per-step kernel)", 1024, 3 << 19, 16, 3, FO2),
    ("16 x 5 -> int16 (window-per-step kernel)", 1024, 5 << 18, 16, 5, FO2),
    ("16 x 32 -> int16 (long)", 1024, 1 << 21, 16, 32, FO2),
    ("64 x 256 -> int16 (long)", 64, 1 << 22, 64, 256, FO2),
    ("1024 x 16 -> int16 (long)", 64, 1 << 20, 1024, 16, FO2),
]


def main():
    only = sys.argv[1] if len(sys.argv) > 1 else None
    for name, n_ch, n, nt, df, fo in SHAPES:
        if only and only not in name:
            continue
        coeffs = np.random.default_rng(nt * 1000 + df).integers(-32768, 32640, size=nt * df, dtype=np.int64)
        arms = [("i16", False), ("s8", True), ("i16_again", False)]
        eng = {}
        for arm, flag in arms:
            eng[arm] = A.PolyDec(nt, df, FIN, FC, FA, fo, n_channels=n_ch, in_bytes=flag)
            eng[arm].set_coeffs(coeffs)
        x16 = torch.empty((n_ch, n), dtype=torch.int16, device="cuda")
        A.fill_stimulus(x16, 0xACD5, 8)
        x8 = x16.to(torch.int8)
        xs = {"i16": x16, "s8": x8, "i16_again": x16}
        no = n // df
        out_eb = A.elem_bytes(fo.W)
        ys = {arm: torch.empty((n_ch, (no + 63) // 64 * 64), dtype=A.torch_dtype_for(fo), device="cuda") for arm, _ in arms}
        ms = {arm: [] for arm, _ in arms}
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(3 * REPS)]
        k = 0
        timed = []
        for r in range(WARMUP + REPS):
            for arm, _ in arms:
                if r >= WARMUP:
                    ev[k][0].record()
                eng[arm].run(xs[arm], ys[arm])
                if r >= WARMUP:
                    ev[k][1].record()
                    timed.append((arm, k))
                    k += 1
        torch.cuda.synchronize()
        for arm, i in timed:
            ms[arm].append(ev[i][0].elapsed_time(ev[i][1]))
        avg = {arm: float(np.mean(v)) for arm, v in ms.items()}
        mn = {arm: float(np.min(v)) for arm, v in ms.items()}
        bps = {"i16": 2 + out_eb / df, "s8": 1 + out_eb / df}

        def gbs(arm, key):
            return bps[key] * n_ch * n / (avg[arm] * 1e-3) / 1e9

        row = {
            "shape": name, "channels": n_ch, "samples": n, "NTAPS": nt, "DF": df, "out_bytes": out_eb,
            "path_i16": eng["i16"].path, "path_s8": eng["s8"].path, "ring_i16": eng["i16"].ring_shape, "ring_s8": eng["s8"].ring_shape,
            "ms_i16_avg": round(avg["i16"], 4), "ms_i16_min": round(mn["i16"], 4),
            "ms_s8_avg": round(avg["s8"], 4), "ms_s8_min": round(mn["s8"], 4),
            "ms_i16_again_avg": round(avg["i16_again"], 4), "ms_i16_again_min": round(mn["i16_again"], 4),
            "ratio_s8_over_i16": round(avg["s8"] / avg["i16"], 4),
            "spread_i16": round(abs(avg["i16_again"] / avg["i16"] - 1.0), 4),
            "expected_if_hbm_bound": round(bps["s8"] / bps["i16"], 4),
            "bytes_per_sample_i16": round(bps["i16"], 4), "bytes_per_sample_s8": round(bps["s8"], 4),
            "gbs_i16": round(gbs("i16", "i16"), 1), "gbs_s8": round(gbs("s8", "s8"), 1),
            "hbm_share_i16": round(gbs("i16", "i16") / HBM_GBS, 3), "hbm_share_s8": round(gbs("s8", "s8") / HBM_GBS, 3),
            "outputs_equal": bool(torch.equal(ys["i16"][:, :no], ys["s8"][:, :no])),
            "timed_calls_per_arm": REPS, "warmup_calls_per_arm": WARMUP,
        }
        print(json.dumps(row), flush=True)
        del eng, x16, x8, xs, ys
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
