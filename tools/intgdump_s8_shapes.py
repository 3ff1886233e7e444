#!/usr/bin/env python3
"""tools/intgdump_s8_shapes.py -- what byte rows (IntgDump(in_bytes=True)) are worth to ac_intg_dump against int16 containers of the same values.

One process.  Per shape three handles on the same 8-bit samples, ACC_TYPE = OUT_TYPE: the flagged one on int8 / uint8 rows, and two unflagged
ones on int16 rows (the path an 8-bit stream takes without the flag) -- the second of them is the same code run again, so the spread between
two runs of one kernel is on record beside the ratio.  The three arms alternate call by call: WARMUP rounds, then REPS timed rounds, every
call one whole-row call of uniform blocks between two events on the stream (the handle has no timers of its own; the events bracket the
kernel launch and nothing else, the block table being the one of the call before).
One JSON line per shape: avg / min ms of the three arms, ratio = s8 / int16 (avg), spread = |int16 second run / int16 - 1|, the path of each
arm, the algorithmic bytes per input sample of both (in_eb + out_eb / NS) and the GB/s they amount to with their share of 8 TB/s, and whether
the outputs are equal."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ac_dsp_amd as A  # noqa: E402

WARMUP, REPS = 3, 20
HBM_GBS = 8000.0
S84, U88 = A.Fmt(8, 4), A.Fmt(8, 8, False)
A32, U32 = A.Fmt(32, 16), A.Fmt(32, 32, False)
N_OBJ, N = 1024, 1 << 20

SHAPES = [
    # name, NS (= rounds of every block), CHN, IN_TYPE, ACC_TYPE = OUT_TYPE
    ("bench geometry: NS 64 CHN 4", 64, 4, S84, A32),
    ("NS 256 CHN 1", 256, 1, S84, A32),
    ("NS 128 CHN 2", 128, 2, S84, A32),
    ("NS 32 CHN 8", 32, 8, S84, A32),
    ("NS 16 CHN 16", 16, 16, S84, A32),
    ("NS 64 CHN 3", 64, 3, S84, A32),
    ("NS 64 CHN 5", 64, 5, S84, A32),
    ("NS 64 CHN 12", 64, 12, S84, A32),
    ("NS 1024 CHN 2", 1024, 2, S84, A32),
    ("NS 16 CHN 1", 16, 1, S84, A32),
    ("unsigned <8,8>: NS 64 CHN 4", 64, 4, U88, U32),
    ("NS 63 CHN 4 (tiled kernel on both arms)", 63, 4, S84, A32),
]


def main():
    only = sys.argv[1] if len(sys.argv) > 1 else None
    for name, ns, chn, fin, fa in SHAPES:
        if only and only not in name:
            continue
        n_blk = N // (ns * chn)
        n = n_blk * ns * chn
        n_sample = np.full(n_blk, ns, dtype=np.int64)
        arms = [("i16", False), ("s8", True), ("i16_again", False)]
        eng = {arm: A.IntgDump(ns, chn, fin, fa, fa, n_objects=N_OBJ, in_bytes=flag) for arm, flag in arms}
        x16 = torch.empty((N_OBJ, N), dtype=torch.int16, device="cuda")
        A.fill_stimulus(x16, 0xACD5, 8)
        if not fin.S:
            x16 = x16 & 0xFF
        x8 = x16.to(eng["s8"].in_dtype)
        xs = {"i16": x16[:, :n], "s8": x8[:, :n], "i16_again": x16[:, :n]}
        ev = {arm: [] for arm, _ in arms}
        ys, paths = {}, {}
        for r in range(WARMUP + REPS):
            for arm, _ in arms:
                # no synchronisation inside the rounds: the host runs ahead of the device, so the two events sit right around the kernel
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ys[arm] = eng[arm].run(xs[arm], n_sample)
                e1.record()
                if r >= WARMUP:
                    ev[arm].append((e0, e1))
                paths[arm] = eng[arm].path
        torch.cuda.synchronize()
        ms = {arm: [a.elapsed_time(b) for a, b in v] for arm, v in ev.items()}
        st = {arm: (sum(v) / len(v), min(v)) for arm, v in ms.items()}
        out_eb = A.elem_bytes(fa.W)
        bps = {"i16": 2 + out_eb / ns, "s8": 1 + out_eb / ns}

        def gbs(arm, key):
            return bps[key] * N_OBJ * n / (st[arm][0] * 1e-3) / 1e9

        row = {
            "shape": name, "objects": N_OBJ, "samples": n, "NS": ns, "CHN": chn, "in": "<%d,%d,%s>" % (fin.W, fin.I, "true" if fin.S else "false"),
            "acc_out": "<%d,%d>" % (fa.W, fa.I), "path_i16": paths["i16"], "path_s8": paths["s8"], "path_i16_again": paths["i16_again"],
            "ms_i16_avg": round(st["i16"][0], 4), "ms_i16_min": round(st["i16"][1], 4),
            "ms_s8_avg": round(st["s8"][0], 4), "ms_s8_min": round(st["s8"][1], 4),
            "ms_i16_again_avg": round(st["i16_again"][0], 4), "ms_i16_again_min": round(st["i16_again"][1], 4),
            "ratio_s8_over_i16": round(st["s8"][0] / st["i16"][0], 4),
            "spread_i16": round(abs(st["i16_again"][0] / st["i16"][0] - 1.0), 4),
            "bytes_per_sample_i16": round(bps["i16"], 4), "bytes_per_sample_s8": round(bps["s8"], 4),
            "gbs_i16": round(gbs("i16", "i16"), 1), "gbs_s8": round(gbs("s8", "s8"), 1),
            "hbm_share_i16": round(gbs("i16", "i16") / HBM_GBS, 3), "hbm_share_s8": round(gbs("s8", "s8") / HBM_GBS, 3),
            "outputs_equal": bool(torch.equal(ys["i16"], ys["s8"])),
            "timed_calls_per_arm": REPS, "warmup_calls_per_arm": WARMUP,
        }
        print(json.dumps(row), flush=True)
        del eng, x16, x8, xs, ys
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
