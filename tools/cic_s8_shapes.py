#!/usr/bin/env python3
"""tools/cic_s8_shapes.py -- what byte rows (Cic(in_bytes=True)) are worth to ac_cic_dec_full against int16 containers of the same values.

One process.  Per shape three handles on the same signed <8,1> samples, OUT_TYPE = INT_TYPE: the flagged one on int8 rows, and two unflagged
ones on int16 rows (the path an 8-bit stream takes without the flag) -- the second of them is the same code run again, so the spread between
two runs of one kernel is on record beside the ratio.  The three arms alternate call by call: WARMUP rounds, then REPS timed rounds; the
times are the handles' own kernel_stats (HIP events around the main kernel).  Every call starts its handle from reset(), so that each timed
call is the same whole-row call at decimation phase 0.
One JSON line per shape: avg / min ms of the three arms, ratio = s8 / int16 (avg), spread = |int16 second run / int16 - 1|, path and
(R1, R2) of both arms, the algorithmic bytes per input sample of both (in_eb + out_eb / R) and the GB/s they amount to with their share of
8 TB/s, the shader clock measured right behind the last call of each arm, and whether the outputs are equal."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

import ac_dsp_amd as A  # noqa: E402

WARMUP, REPS = 3, 20
FIN = A.Fmt(8, 1)
HBM_GBS = 8000.0

SHAPES = [
    # name, channels, samples, R, M, N
    ("cic_dec_r64 geometry", 4096, 1 << 20, 64, 1, 4),
    ("R 32 N 4", 1024, 1 << 20, 32, 1, 4),
    ("R 256 N 3", 1024, 1 << 20, 256, 1, 3),
    ("R 128 M 2 N 3", 1024, 1 << 20, 128, 2, 3),
    ("R 24 N 4 (s8_r8)", 1024, 1 << 20, 24, 1, 4),
    ("R 12 N 5 (s8_r4)", 1024, 1 << 20, 12, 1, 5),
    ("R 8 N 2 (s8_r4)", 1024, 1 << 20, 8, 1, 2),
    ("R 244 M 2 N 3 (s8_r4, two warm-up steps)", 1024, 1 << 20, 244, 2, 3),
    ("R 37 N 3 (recurrence on both arms)", 1024, 1 << 20, 37, 1, 3),
]


def main():
    only = sys.argv[1] if len(sys.argv) > 1 else None
    for name, n_ch, n, R, M, N in SHAPES:
        if only and only not in name:
            continue
        it = A.Cic(False, R, M, N, FIN, FIN).int_type
        fout = A.Fmt(it.W, it.I)
        arms = [("i16", False), ("s8", True), ("i16_again", False)]
        eng = {arm: A.Cic(False, R, M, N, FIN, fout, n_channels=n_ch, in_bytes=flag) for arm, flag in arms}
        x16 = torch.empty((n_ch, n), dtype=torch.int16, device="cuda")
        A.fill_stimulus(x16, 0xACD5, 8)
        x8 = x16.to(torch.int8)
        xs = {"i16": x16, "s8": x8, "i16_again": x16}
        no = eng["i16"].out_count(n)
        out_eb = A.elem_bytes(fout.W)
        per64 = max(1, 64 // out_eb)
        ys = {arm: torch.empty((n_ch, (no + per64 - 1) // per64 * per64), dtype=A.torch_dtype_for(fout), device="cuda") for arm, _ in arms}
        clock, paths = {}, {}
        for r in range(WARMUP + REPS):
            for arm, _ in arms:
                eng[arm].reset()
                eng[arm].run(xs[arm], ys[arm])
                if r == WARMUP + REPS - 1:
                    clock[arm] = A.diag_shader_clock_mhz(0)
                    paths[arm] = eng[arm].path
        torch.cuda.synchronize()
        st = {arm: eng[arm].kernel_stats(REPS) for arm, _ in arms}
        bps = {"i16": 2 + out_eb / R, "s8": 1 + out_eb / R}

        def gbs(arm, key):
            return bps[key] * n_ch * n / (st[arm][0] * 1e-3) / 1e9

        row = {
            "shape": name, "channels": n_ch, "samples": n, "R": R, "M": M, "N": N, "out": "<%d,%d>" % (fout.W, fout.I), "out_bytes": out_eb,
            "path_i16": paths["i16"], "path_s8": paths["s8"],
            "rates_i16": list(eng["i16"].two_stage_rates), "rates_s8": list(eng["s8"].two_stage_rates),
            "ms_i16_avg": round(st["i16"][0], 4), "ms_i16_min": round(st["i16"][1], 4),
            "ms_s8_avg": round(st["s8"][0], 4), "ms_s8_min": round(st["s8"][1], 4),
            "ms_i16_again_avg": round(st["i16_again"][0], 4), "ms_i16_again_min": round(st["i16_again"][1], 4),
            "ratio_s8_over_i16": round(st["s8"][0] / st["i16"][0], 4),
            "spread_i16": round(abs(st["i16_again"][0] / st["i16"][0] - 1.0), 4),
            "bytes_per_sample_i16": round(bps["i16"], 4), "bytes_per_sample_s8": round(bps["s8"], 4),
            "gbs_i16": round(gbs("i16", "i16"), 1), "gbs_s8": round(gbs("s8", "s8"), 1),
            "hbm_share_i16": round(gbs("i16", "i16") / HBM_GBS, 3), "hbm_share_s8": round(gbs("s8", "s8") / HBM_GBS, 3),
            "clock_mhz_i16": round(clock["i16"], 1), "clock_mhz_s8": round(clock["s8"], 1), "clock_mhz_i16_again": round(clock["i16_again"], 1),
            "outputs_equal": bool(torch.equal(ys["i16"][:, :no], ys["s8"][:, :no])),
            "timed_calls_per_arm": REPS, "warmup_calls_per_arm": WARMUP,
        }
        print(json.dumps(row), flush=True)
        del eng, x16, x8, xs, ys
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
