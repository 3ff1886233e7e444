"""Node-level sharding of the polydec cascade (acdsp_node_ddc_create_polydec): the bank cut into contiguous channel slices on one device, every
slice against the oracle cascade run over the whole, unsharded bank -- two calls, the first leaving a word waiting in every shard."""
import numpy as np
import pytest

import ac_dsp_amd as A
from ddc_polydec_ref import oracle_cascade, polydec_coeffs
from oracle import stimulus

pytestmark = pytest.mark.gpu

SEED = 0xACD5


def test_polydec_ddc_bank_on_three_shards_of_one_device():
    cin, fc, fa, fo = A.Fmt(16, 1), A.Fmt(16, 1), A.Fmt(60, 30), A.Fmt(24, 9, True, "RND", "SAT")
    n_ch, cut, n = 10, 16 * 2049, 16 * 4096
    c = polydec_coeffs(64, 2, fc)
    node = A.NodeDdcPolyDec(16, 1, 5, cin, 64, 2, fc, fa, fo, n_ch, [0, 0, 0])
    assert node.slices == [A.node_shard(n_ch, 3, s) for s in range(3)]
    node.set_coeffs(c)
    xs = node.alloc(cin, n, lambda t, lo: A.fill_stimulus(t, SEED, 16, ch0=lo))
    outs = []
    for a, b in ((0, cut), (cut, n)):
        ys = node.run([x[:, a:b] for x in xs])
        outs.append(np.concatenate([y.cpu().numpy().astype(np.int64) for y in ys], axis=0))
    got = np.concatenate(outs, axis=1)
    want = oracle_cascade(16, 1, 5, cin, node.int_type, 64, 2, fc, fa, fo, c, stimulus(SEED, n_ch, n, 16), [cut])
    assert outs[0].shape[1] == 1024 and got.shape == want.shape and np.array_equal(got, want)
