#!/usr/bin/env python3
"""tools/mvavg_s8_shapes.py -- what byte rows (MvAvg(in_bytes=True[, out_bytes=True])) are worth to ac_mv_avg against int16 containers of the same values.

One process.  Per shape four handles on the same 8-bit samples and the same 8-bit OUT_TYPE: int16 -> int16 (unflagged: the path an 8-bit stream
takes without the flags), bytes -> int16 (ACDSP_FLAG_IN_BYTES), bytes -> bytes (both flags), and the unflagged one again -- the same code run a
second time, so the spread between two runs of one kernel is on record beside the ratios.  The four arms alternate call by call: WARMUP rounds,
then REPS timed rounds, every call one whole-row call between two events on the stream (no synchronisation inside the rounds: the host runs
ahead of the device, so the events sit right around the kernel).  512 objects x 2^20 samples in frames of 1024: 0.5 / 1 GB in, as much out.
One JSON line per shape: avg / min ms of the arms, ratio of each flagged arm to the int16 arm (avg) beside its floor by bytes (0.75 / 0.50),
spread = |int16 second run / int16 - 1|, the path of each arm, the GB/s of each arm's algorithmic bytes with their share of 8 TB/s, and whether
the flagged arms' words equal the int16 arm's."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ac_dsp_amd as A  # noqa: E402

WARMUP, REPS = 3, 20
HBM_GBS = 8000.0
N_OBJ, N, FRAME = 512, 1 << 20, 1024
S84 = A.Fmt(8, 4)
FC = A.Fmt(16, 8)                      # F = 8: unit gain = 256
ACC_LIN = A.Fmt(40, 26)                # F = 14 = F_in + F_coeff + 2: the linear class
ACC_TAP = A.Fmt(32, 24)                # F = 8 < F_in + F_coeff: every product loses bits (the per-tap class, off the matrix cores)
OUT = A.Fmt(8, 4, True, "RND", "SAT")


def box(taps):
    """box weights of unit gain: one signed byte each (no high digit)"""
    c = np.full(taps, 256 // taps, dtype=np.int64)
    c[taps // 2] += 256 - c.sum()
    return c


def hann_hi(taps):
    """a Hann window of gain 16: its centre weights need a high digit"""
    w = np.hanning(taps + 2)[1:-1]
    return np.round(w / w.sum() * 4096).astype(np.int64)


SHAPES = [("%d taps %s, box weights" % (t, m), t, m, box, ACC_LIN) for m in ("MIRROR", "WIN") for t in (3, 9, 17, 33, 65)] + [
    ("33 taps MIRROR, Hann weights of gain 16 (high digits)", 33, "MIRROR", hann_hi, ACC_LIN),
    ("9 taps MIRROR, per-tap class (ACC <32,24>: the order-free int64 kernel on byte rows)", 9, "MIRROR", box, ACC_TAP),
]
ARMS = [("i16", False, False), ("s8_i16", True, False), ("s8_s8", True, True), ("i16_again", False, False)]


def main():
    only = sys.argv[1] if len(sys.argv) > 1 else None
    x16 = torch.empty((N_OBJ, N), dtype=torch.int16, device="cuda")
    A.fill_stimulus(x16, 0xACD5, 8)
    x8 = x16.to(torch.int8)
    for name, taps, mode, cset, fa in SHAPES:
        if only and only not in name:
            continue
        c = cset(taps)
        eng = {}
        for arm, ib, ob in ARMS:
            eng[arm] = A.MvAvg(FRAME, taps, mode, S84, FC, fa, OUT, n_objects=N_OBJ, in_bytes=ib, out_bytes=ob)
            eng[arm].set_coeffs(c)
        no = eng["i16"].out_per_frame(FRAME) * (N // FRAME)
        xs = {arm: (x8 if ib else x16) for arm, ib, _ in ARMS}
        ys = {arm: torch.empty((N_OBJ, N), dtype=eng[arm].out_dtype, device="cuda") for arm, _, _ in ARMS}
        ev = {arm: [] for arm, _, _ in ARMS}
        paths = {}
        for r in range(WARMUP + REPS):
            for arm, _, _ in ARMS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                eng[arm].run(xs[arm], FRAME, out=ys[arm])
                e1.record()
                if r >= WARMUP:
                    ev[arm].append((e0, e1))
                paths[arm] = eng[arm].path
        torch.cuda.synchronize()
        ms = {arm: [a.elapsed_time(b) for a, b in v] for arm, v in ev.items()}
        st = {arm: (sum(v) / len(v), min(v)) for arm, v in ms.items()}
        bps = {"i16": 2 + 2 * no / N, "s8_i16": 1 + 2 * no / N, "s8_s8": 1 + 1 * no / N, "i16_again": 2 + 2 * no / N}

        def gbs(arm):
            return bps[arm] * N_OBJ * N / (st[arm][0] * 1e-3) / 1e9

        ref = ys["i16"][:, :no]
        row = {"shape": name, "objects": N_OBJ, "samples": N, "frame": FRAME, "taps": taps, "mode": mode, "acc": "<%d,%d>" % (fa.W, fa.I),
               "sum_abs_c": int(np.abs(c).sum()), "high_digit": bool((np.abs(c) > 127).any())}
        for arm, _, _ in ARMS:
            row["path_" + arm] = paths[arm]
            row["ms_%s_avg" % arm] = round(st[arm][0], 4)
            row["ms_%s_min" % arm] = round(st[arm][1], 4)
            row["gbs_" + arm] = round(gbs(arm), 1)
            row["hbm_share_" + arm] = round(gbs(arm) / HBM_GBS, 3)
        row["ratio_s8_i16_over_i16"] = round(st["s8_i16"][0] / st["i16"][0], 4)
        row["floor_s8_i16"] = round(bps["s8_i16"] / bps["i16"], 3)
        row["ratio_s8_s8_over_i16"] = round(st["s8_s8"][0] / st["i16"][0], 4)
        row["floor_s8_s8"] = round(bps["s8_s8"] / bps["i16"], 3)
        row["spread_i16"] = round(abs(st["i16_again"][0] / st["i16"][0] - 1.0), 4)
        row["outputs_equal"] = bool(torch.equal(ref, ys["s8_i16"][:, :no]) and torch.equal(ref, ys["s8_s8"][:, :no].to(torch.int16)))
        row["timed_calls_per_arm"], row["warmup_calls_per_arm"] = REPS, WARMUP
        print(json.dumps(row), flush=True)
        del eng, ys
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
