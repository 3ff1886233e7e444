#!/usr/bin/env python3
"""tools/ddc_polydec_shapes.py -- what the fused polydec cascade (DdcPolyDec, acdsp_ddc_create_polydec) is worth against the two ways the
chain ac_cic_dec_full -> ac_poly_dec ran before it.

One process.  Per shape three arms on the same int16 rows, each arm TWICE (a second handle of the same kind: the spread between two runs of
one code path is on record beside every ratio):
  a  the fused composite, DdcPolyDec at DF 2 with a 128-tap prototype (NTAPS 64);
  b  a Cic handle into a PolyDec handle through an INT_TYPE buffer in HBM (the word count is even: no leftover to queue);
  c  today's fused Ddc at FULL rate with the same 128-tap prototype as a FIR, every second output being the chain's.
The bench.py `ddc` types: <16,1> samples, INT_TYPE <36,21>, <16,1> coefficients, <60,30> sums, OUT <24,9,RND,SAT>.  The six handles alternate
call by call: WARMUP rounds, then REPS timed rounds; ms per call are torch stream events around the whole call (both kernels of arm b, the
history updates behind every main kernel).  Every call starts its handles from reset(), so each timed call is the same whole-row call at
decimation phase 0 with an empty queue.
One JSON line per shape: avg / min ms of the arms, spread_x = |second handle / first handle - 1| of arm x, the ratios a/b and a/c (avg of the
first handles), faster_than_b = a/b < 1 - max(spread_a, spread_b), the algorithmic HBM bytes per intermediate word of every arm with the
GB/s they amount to, and whether the outputs agree (a == b word for word, a == every second output of c)."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ac_dsp_amd as A  # noqa: E402
from bench import windowed_sinc_raw  # noqa: E402

WARMUP, REPS = 3, 20
FIN, FC, FA, FO = A.Fmt(16, 1), A.Fmt(16, 1), A.Fmt(60, 30), A.Fmt(24, 9, True, "RND", "SAT")
R, N, NTAPS, DF = 16, 5, 64, 2

# name, channels, samples (the bench.py `ddc` row, and 512 streams of the same length)
SHAPES = [
    ("bench.py ddc geometry", 4096, 1 << 20),
    ("512 streams", 512, 1 << 20),
]


class Pair:
    """arm b: Cic -> PolyDec through a buffer of INT_TYPE words"""

    def __init__(self, n_ch, n, c, mid):
        self.cic = A.Cic(False, R, 1, N, FIN, mid, n_channels=n_ch)
        self.pd = A.PolyDec(NTAPS, DF, mid, FC, FA, FO, n_channels=n_ch)
        self.pd.set_coeffs(c)
        self.mid = torch.empty((n_ch, n // R), dtype=torch.int64, device="cuda")

    def reset(self):
        self.cic.reset()
        self.pd.reset()

    def run(self, x, y):
        return self.pd.run(self.cic.run(x, self.mid), y)

    path = property(lambda self: "%s+%s" % (self.cic.path, self.pd.path))


def main():
    only = sys.argv[1] if len(sys.argv) > 1 else None
    h = np.concatenate([windowed_sinc_raw(NTAPS * DF - 1, 0.1, FC.F), [0]]).astype(np.int64)   # the prototype, 128 taps
    c = np.array([h[tp * DF + d] for d in range(DF) for tp in range(NTAPS)], dtype=np.int64)    # c[tp + NTAPS d] = h[tp DF + d]
    for name, n_ch, n in SHAPES:
        if only and only not in name:
            continue
        arms = ["a", "b", "c", "a_again", "b_again", "c_again"]
        eng = {}
        for k in ("a", "a_again"):
            eng[k] = A.DdcPolyDec(R, 1, N, FIN, NTAPS, DF, FC, FA, FO, n_channels=n_ch)
            eng[k].set_coeffs(c)
        mid = eng["a"].int_type
        for k in ("b", "b_again"):
            eng[k] = Pair(n_ch, n, c, mid)
        for k in ("c", "c_again"):
            eng[k] = A.Ddc(R, 1, N, FIN, NTAPS * DF, "SHIFT_REG", FC, FA, FO, n_channels=n_ch)
            eng[k].set_coeffs(h)
        x = torch.empty((n_ch, n), dtype=torch.int16, device="cuda")
        A.fill_stimulus(x, 0xACD5, 16)
        n_mid = n // R
        no = {k: (n_mid if k.startswith("c") else n_mid // DF) for k in arms}
        ys = {k: torch.empty((n_ch, (no[k] + 7) // 8 * 8), dtype=torch.int32, device="cuda") for k in arms}
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)] for k in arms}
        for r in range(WARMUP + REPS):
            for k in arms:
                eng[k].reset()
                if r >= WARMUP:
                    ev[k][r - WARMUP][0].record()
                eng[k].run(x, ys[k])
                if r >= WARMUP:
                    ev[k][r - WARMUP][1].record()
        torch.cuda.synchronize()
        ms = {k: [a.elapsed_time(b) for a, b in ev[k]] for k in arms}
        avg = {k: sum(ms[k]) / REPS for k in arms}
        spread = {k: abs(avg[k + "_again"] / avg[k] - 1.0) for k in ("a", "b", "c")}
        # HBM bytes per intermediate word: R int16 samples in; 8 written + 8 re-read between the kernels of b; 4 / DF out (c: 4 out)
        bpw = {"a": 2 * R + 4 / DF, "b": 2 * R + 16 + 4 / DF, "c": 2 * R + 4}
        gbs = {k: bpw[k] * n_ch * n_mid / (avg[k] * 1e-3) / 1e9 for k in ("a", "b", "c")}
        ya = ys["a"][:, :no["a"]]
        equal_ab = bool(torch.equal(ya, ys["b"][:, :no["b"]]))
        equal_ac = bool(torch.equal(ya, ys["c"][:, DF - 1:n_mid:DF]))
        r_ab, r_ac = avg["a"] / avg["b"], avg["a"] / avg["c"]
        row = {
            "shape": name, "channels": n_ch, "samples": n, "R": R, "N": N, "ntaps": NTAPS, "df": DF, "int_type": repr(mid), "out": repr(FO),
            "path_a": eng["a"].path, "path_b": eng["b"].path, "path_c": eng["c"].path,
            "ms_avg": {k: round(avg[k], 4) for k in arms}, "ms_min": {k: round(min(ms[k]), 4) for k in arms},
            "kernel_ms_a": round(eng["a"].kernel_stats(REPS)[0], 4), "kernel_ms_c": round(eng["c"].kernel_stats(REPS)[0], 4),
            "spread": {k: round(v, 4) for k, v in spread.items()},
            "ratio_a_over_b": round(r_ab, 4), "ratio_a_over_c": round(r_ac, 4),
            "faster_than_b": bool(r_ab < 1.0 - max(spread["a"], spread["b"])), "faster_than_c": bool(r_ac < 1.0 - max(spread["a"], spread["c"])),
            "bytes_per_word": bpw, "expected_a_over_b_by_bytes": round(bpw["a"] / bpw["b"], 4), "gbs": {k: round(v, 1) for k, v in gbs.items()},
            "outputs_a_equal_b": equal_ab, "outputs_a_equal_c_decimated": equal_ac, "timed_calls_per_arm": REPS, "warmup_calls_per_arm": WARMUP,
        }
        print(json.dumps(row), flush=True)
        assert equal_ab and equal_ac, "the arms disagree on " + name
        del eng, x, ys
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
