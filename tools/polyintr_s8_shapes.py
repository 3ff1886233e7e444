#!/usr/bin/env python3
"""tools/polyintr_s8_shapes.py -- what byte rows (PolyIntr(in_bytes=True[, out_bytes=True])) are worth to ac_poly_intr against int16 containers of
the same values.

One process.  Per shape four handles on the same 8-bit samples and the same 8-bit OUT_TYPE: int16 -> int16 (unflagged: the path an 8-bit stream
takes without the flags), bytes -> int16 (ACDSP_FLAG_IN_BYTES), bytes -> bytes (both flags), and the unflagged one again -- the same code run a
second time, so the spread between two runs of one kernel is on record beside the ratios.  The four arms alternate call by call: WARMUP rounds,
then REPS timed rounds, every call one whole-row call between two events on the stream (no synchronisation inside the rounds: the host runs
ahead of the device, so the events sit around the call's kernels -- the matrix-core kernel with the head / tail kernels on the side stream).
1024 channels x 2^18 input samples, the geometry of bench.py's polyintr row; its coefficient set and control words on the IF = 8 rows.
One JSON line per shape: avg / min ms of the arms, ratio of each flagged arm to the int16 arm (avg) beside its floor by bytes, spread =
|int16 second run / int16 - 1|, the path of each arm, the GB/s of each arm's algorithmic bytes with their share of 8 TB/s, and whether the
flagged arms' words equal the int16 arm's."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ac_dsp_amd as A  # noqa: E402

WARMUP, REPS = 3, 20
HBM_GBS = 8000.0
N_CH, N = 1024, 1 << 18
S82 = A.Fmt(8, 2)
FC = A.Fmt(16, 2)
ACC_32 = A.Fmt(32, 12)                 # F = 20 = F_in + F_coeff: the 32-bit epilogue
ACC_40 = A.Fmt(40, 12)                 # F = 28 (bench.py's ACC_TYPE): a left shift into ACC_TYPE, the generic epilogue
OUT = A.Fmt(8, 2, True, "RND", "SAT")


def windowed_sinc_raw(n_taps, cutoff, frac_bits):
    """bench.py's low-pass: Hamming-windowed sinc of unit gain, made exactly symmetric"""
    k = np.arange(n_taps) - (n_taps - 1) / 2.0
    win = 0.54 - 0.46 * np.cos(2 * np.pi * np.arange(n_taps) / (n_taps - 1))
    h = np.sinc(2 * cutoff * k) * 2 * cutoff * win
    raw = np.round(h / h.sum() * 2.0 ** frac_bits).astype(np.int64)
    return (raw + raw[::-1]) // 2


def lowpass(ifac):
    """FOLD_EVEN, 16 taps: 8 IF coefficients; IF = 8 is bench.py's set"""
    if ifac == 8:
        return windowed_sinc_raw(127, 0.05, 14)[:64]
    return windowed_sinc_raw(16 * ifac - 1, 0.4 / ifac, 14)[:8 * ifac]


def plain(ifac):
    return [1] * ifac, list(range(ifac))


def pairs(ifac):
    return [1] * ifac, [ifac - 1 - j for j in range(ifac)]


def full_range(count):
    return np.random.default_rng(5).integers(-32768, 32768, size=count, dtype=np.int64)


# (name, NTAPS, IF, ftype, coefficients, (sign, corr), ACC_TYPE)
SHAPES = [
    ("bench set, IF 8, ACC <32,12> (32-bit epilogue)", 16, 8, "FOLD_EVEN", lowpass(8), plain(8), ACC_32),
    ("bench set, IF 8, ACC <40,12> (generic epilogue)", 16, 8, "FOLD_EVEN", lowpass(8), plain(8), ACC_40),
    ("low-pass, IF 2, ACC <32,12>", 16, 2, "FOLD_EVEN", lowpass(2), plain(2), ACC_32),
    ("low-pass, IF 4, ACC <32,12>", 16, 4, "FOLD_EVEN", lowpass(4), plain(4), ACC_32),
    ("low-pass, IF 16, ACC <32,12>", 16, 16, "FOLD_EVEN", lowpass(16), plain(16), ACC_32),
    ("low-pass, IF 6 (24 live rows of 32), ACC <32,12>", 16, 6, "FOLD_EVEN", lowpass(6), plain(6), ACC_32),
    ("symmetric pairs, full-range taps (three digit planes), IF 8, ACC <32,12>", 16, 8, "FOLD_EVEN", full_range(64), pairs(8), ACC_32),
    ("FOLD_ANTI 40 taps (two K blocks), IF 4, ACC <32,12>", 40, 4, "FOLD_ANTI", full_range(160) // 4, plain(4), ACC_32),
]
ARMS = [("i16", False, False), ("s8_i16", True, False), ("s8_s8", True, True), ("i16_again", False, False)]


def main():
    only = sys.argv[1] if len(sys.argv) > 1 else None
    x16 = torch.empty((N_CH, N), dtype=torch.int16, device="cuda")
    A.fill_stimulus(x16, 0xACD5, 8)
    x8 = x16.to(torch.int8)
    for name, n_taps, ifac, ftype, c, (sign, corr), fa in SHAPES:
        if only and only not in name:
            continue
        eng = {}
        for arm, ib, ob in ARMS:
            eng[arm] = A.PolyIntr(n_taps, len(c), ifac, ftype, S82, FC, fa, OUT, n_channels=N_CH, in_bytes=ib, out_bytes=ob)
            eng[arm].set_ctrl(c, sign, corr)
        xs = {arm: (x8 if ib else x16) for arm, ib, _ in ARMS}
        no = N * ifac
        ys = {arm: torch.empty((N_CH, no), dtype=eng[arm].out_dtype, device="cuda") for arm, _, _ in ARMS}
        for arm, _, _ in ARMS:
            eng[arm].run(xs[arm][:, :16])           # past the stream's first sample: every later call emits IF per input
        ev = {arm: [] for arm, _, _ in ARMS}
        paths = {}
        for r in range(WARMUP + REPS):
            for arm, _, _ in ARMS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                eng[arm].run(xs[arm], out=ys[arm])
                e1.record()
                if r >= WARMUP:
                    ev[arm].append((e0, e1))
                paths[arm] = eng[arm].path
        torch.cuda.synchronize()
        ms = {arm: [a.elapsed_time(b) for a, b in v] for arm, v in ev.items()}
        st = {arm: (sum(v) / len(v), min(v)) for arm, v in ms.items()}
        bps = {"i16": 2 + 2 * ifac, "s8_i16": 1 + 2 * ifac, "s8_s8": 1 + ifac, "i16_again": 2 + 2 * ifac}

        def gbs(arm):
            return bps[arm] * N_CH * N / (st[arm][0] * 1e-3) / 1e9

        # every arm has consumed the same stream (the same rows WARMUP + REPS times): the last call's outputs must agree word for word
        row = {"shape": name, "channels": N_CH, "samples": N, "taps": n_taps, "ifac": ifac, "ftype": ftype, "acc": "<%d,%d>" % (fa.W, fa.I),
               "max_abs_c": int(np.abs(c).max())}
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
        eq = torch.equal(ys["i16"], ys["s8_i16"])
        half = N_CH // 2                                 # (the widened copy of the byte rows in two halves: 4 GB at IF 16)
        for lo in (0, half):
            eq = eq and torch.equal(ys["i16"][lo:lo + half], ys["s8_s8"][lo:lo + half].to(torch.int16))
        row["outputs_equal"] = bool(eq)
        row["timed_calls_per_arm"], row["warmup_calls_per_arm"] = REPS, WARMUP
        print(json.dumps(row), flush=True)
        del eng, ys
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
