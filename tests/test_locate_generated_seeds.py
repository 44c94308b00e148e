"""The planted damage of tests/test_gpu_locate_generated.py::test_every_layout,
checked on the CPU: the same draws (damage_every_code on the same seeds) turned
into syndromes directly -- a hit of data row r adds c[:, r] x to the column, a
hit of parity row k + p adds x to syndrome p -- and given to the numpy model
(tests/locate_model.py).  What the GPU test asserts of the model must hold for
the seeds it commits: on a Cauchy matrix every block damaged in n <= min(u, e -
1) rows lists exactly the planted rows, on the gf_gen_rs_matrix codes at least
three quarters of them are located, and the two over-damaged blocks are
DAMAGED."""
import numpy as np
import pytest

pytest.importorskip("torch")

import degraded_model as dm  # noqa: E402
import gpu_family as gf  # noqa: E402
import locate_model as lm  # noqa: E402
import scrub_model as sm  # noqa: E402
from test_gpu_locate_fused import damage_every_code  # noqa: E402
from test_gpu_locate_generated import L0, MATRICES  # noqa: E402


class Syndromes:
    """The blocks' syndromes (B, e, L) under damage_every_code's hits."""

    def __init__(self, k, e, L, B, kind):
        self.k, self.c = k, gf.matrix(k, e, kind)
        self.syn = np.zeros((B, e, L), np.uint8)

    def hit(self, rng, blk, row, cols):  # Blocks.hit's draws, in its order
        cols = np.asarray(cols, np.int64)
        x = rng.integers(1, 256, len(cols)).astype(np.uint8)
        if row < self.k:
            self.syn[blk][:, cols] ^= sm.gf_mul(self.c[:, row][:, None], x[None, :])
        else:
            self.syn[blk][row - self.k, cols] ^= x


@pytest.mark.parametrize("kind", ["cauchy", "rs"])
@pytest.mark.parametrize("k,e", MATRICES, ids=str)
def test_the_model_on_the_committed_seeds(k, e, kind):
    st = Syndromes(k, e, L0, 8, kind)
    rows = damage_every_code(st, np.random.default_rng(100 * k + e), k, e, L0)
    for u in (1, 3, 8):
        want = [lm.report_syn(st.c, s, u) for s in st.syn]
        assert want[0][0] == want[7][0] == (0, lm.CLEAN, -1)
        within = [b for b in range(1, 6) if len(rows[b]) <= min(u, e - 1)]
        assert within
        if kind == "cauchy":
            for b in within:
                assert list(map(int, want[b][1])) == rows[b] + [dm.NONE] * (u - len(rows[b])), (u, b)
        else:
            located = [b for b in within if want[b][0][1] in (lm.ONE_ROW, lm.ROWS)]
            assert 4 * len(located) >= 3 * len(within), (u, within, located)
        assert want[5][0][1] == want[6][0][1] == lm.DAMAGED
