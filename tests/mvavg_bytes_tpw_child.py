"""Child process of tests/test_mvavg_bytes_gpu.py::test_runs_of_tiles_per_wave: the parent sets ACDSP_MVAVG_TPW (read once per process), so that
a wave of mv_avg_s8_kernel walks a run of tiles across frame and object boundaries at row lengths a test can afford -- by itself the launcher
gives a wave more than one tile only from 16384 tiles on.  Prints one line per case and "OK" when every word equals the oracle's."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from helpers import rand_fmt                                              # noqa: E402
from test_mvavg_bytes_gpu import F, N_OBJ, acc_for, make, oracle, to_dev, weights, words   # noqa: E402


def main():
    assert int(os.environ["ACDSP_MVAVG_TPW"]) > 1
    rng = np.random.default_rng(int(os.environ["ACDSP_MVAVG_TPW"]))
    bad = 0
    # 1040-sample frames are three tiles (512, 512, 16 outputs), 3 frames x 5 objects = 45 tiles: runs of 3 / 7 / 64 tiles end inside frames and objects
    for taps, mode, fin, fo, ob in ((35, "MIRROR", F(8, 4), F(8, 4, True, "RND", "SAT"), True), (9, "WIN", F(8, 8, False), F(16, 10, True, "RND", "SAT"), False),
                                    (65, "CLIP", F(8, 4), F(24, 12, True, "TRN", "WRAP"), False), (3, "WIN", F(5, 5, False), F(8, 8, False, "TRN", "WRAP"), True)):
        c, n, frames = weights(rng, taps, 256), 1040, 3
        x = rand_fmt(rng, fin, (N_OBJ, n * frames))
        eng = make(taps, mode, fin, acc_for(fin), fo, c, out_bytes=ob)
        y = words(eng.run(to_dev(x, eng.in_dtype), n))
        want = oracle(taps, mode, fin, acc_for(fin), fo).run(c, x, n)
        diff = int((y != want).sum()) if y.shape == want.shape else -1
        print("taps %d %s out_bytes %s: path %s, %d words differ" % (taps, mode, ob, eng.path, diff))
        bad += diff != 0 or eng.path != "stream_s8"
    torch.cuda.synchronize()
    print("OK" if not bad else "FAILED")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
