"""The shapes, lengths and damage of the generated scrub family at wide k and
wide e together (k_rs_jit_* / k_rs_jitw_* scrub, repair, locate, degraded and
correct behind rsgpu_set_scrub_kernel GENERATED): more than 64 source rows on
every layout of the generated kernels, where the strided loops over the rows
take a second and a third trip, the row tables are read at rows >= 64 and >=
128 and the LDS budgets that depend on k are nearly or wholly used.  Not a
test module: tests/test_family_wide_cases.py (the models alone) and
tests/test_gpu_family_generated_wide.py (the device) import it.

Damage is [(row, column, x)] per block: byte `column` of row `row` (source, or
parity from k on) is XORed with x.  The models are run on syndromes, and the
ones that write rows (repair, correct) on the bad columns alone: every verdict
of theirs is per column, so the clean columns add nothing but time."""
import os
from collections import namedtuple

import numpy as np

import correct_cases as cc
import correct_generated_cases as gc
import correct_model as cm
import degraded_model as dm
import gpu_family as gf
import locate_model as lm
import repair_model as rm
import scrub_model as sm

TILE = 2048
L0 = gc.L0  # three full tiles and five lanes
LENGTHS = (L0, 32)  # and one live lane
B = 8
US = (1, 3, 8)  # the locate's list lengths

# (k, e, matrix): Cauchy, or gf_gen_rs_matrix passed as the caller's `coef` so
# that no compiled kernel takes precedence.  The smallest k that reaches each
# edge, and no multiple of the layout's chunk (8, 5, 6 sources for 8, 10 and
# 12 / 16 rows per wave) but for the three shapes that are what they are.
SHAPES = [
    (65, 6, "cauchy"),    # 1 wave x 8 rows: one lane on the second trip
    (70, 12, "cauchy"),   # 2 x 8
    (66, 20, "cauchy"),   # 2 x 10
    (100, 20, "rs"),      # 2 x 10: the C5 code (k = 20 chunks of 5, as the benchmark runs it)
    (67, 24, "cauchy"),   # 2 x 12
    (129, 32, "cauchy"),  # 2 x 16: three trips, the last with one lane
    (218, 32, "rs"),      # 2 x 16: k + e = 250
    (131, 34, "cauchy"),  # 4 x 10: rows >= 128 (130 is 26 chunks of 5: one more)
    (70, 44, "cauchy"),   # 4 x 12
    (201, 49, "cauchy"),  # 4 x 16: the largest k of the layout
    (151, 64, "cauchy"),  # 4 x 16: the last k whose pair tables fit at e = 64 (24552 of 24576 bytes)
    (152, 64, "cauchy"),  # 4 x 16: the first that does not: t = 2 runs TWO_PASS
    (183, 60, "cauchy"),  # the same line at e = 60
    (184, 60, "cauchy"),
    (186, 64, "cauchy"),  # k + e = 250 at e = 64 (31 chunks of 6: the sum fixes k); t = 2 runs TWO_PASS
]
# the shapes whose pair tables do not fit (fits, below): t = 2 runs TWO_PASS
NO_FIT = [(152, 64), (184, 60), (186, 64)]
# one two-wave shape per row count, also run with 2 and 3 tiles per workgroup
TILED = [(66, 20, "cauchy"), (67, 24, "cauchy"), (129, 32, "cauchy")]
CALLS = ("scrub", "repair", "locate", "degraded", "correct")


def layout(e):
    """(waves, rows per wave) of the generated kernels' tile at e parity rows."""
    assert 1 <= e <= 64
    if e <= 16:
        return (1 if e <= 8 else 2), 8
    if e <= 32:
        return 2, 16 if e > 24 else 12 if e > 20 else 10
    return 4, 16 if e > 48 else 12 if e > 40 else 10


LAYOUTS = [(1, 8), (2, 8), (2, 10), (2, 12), (2, 16), (4, 10), (4, 12), (4, 16)]


def fits(k, e, t=2):
    """csrc/rs_jit.hip jit_correct_fits, which tests/test_family_wide_cases.py
    compares with this through the test hooks: four waves of 16 rows hold
    3336 + 256 e + 32 k bytes of tables in 24576 bytes of chunk buffers."""
    return t != 2 or e <= 48 or 256 * e + 32 * k <= 21240


def random_locatable(k, e, rng):
    """A random e x k matrix that rsgpu_scrub_locatable accepts: rows 0 and 1
    without a zero and with k distinct ratios (drawn as such: k random bytes
    do not have distinct ratios from about k = 40 on), the other rows any
    bytes."""
    c = rng.integers(0, 256, (e, k), dtype=np.uint8)
    c[0] = rng.integers(1, 256, k)
    c[1] = sm.gf_mul(c[0], (1 + rng.permutation(255)[:k]).astype(np.uint8))
    return c


def matrix(k, e, kind, seed=0):
    if kind == "random":
        rng = np.random.default_rng(70000 + seed)
        c = random_locatable(k, e, rng)
        while not sm.locatable(c):
            c = random_locatable(k, e, rng)
        return c
    return gf.matrix(k, e, kind)


def columns(L, i):
    """The columns of the i-th damaged row of a block (i < 10), no two rows of
    a block sharing one: in the first tile, a middle tile and the last
    (partial) tile of a row of three tiles or more, three spread over a
    shorter row; the first row of a block also the row's first and last
    byte."""
    assert 0 <= i < 10 and L % 32 == 0 and L > 0
    if L >= 3 * TILE:
        last = (L - 1) // TILE * TILE
        mid = TILE * (1 + i % (last // TILE - 1))
        cols = [5 + 37 * i, mid + 1000 + 41 * i, last + (7 + 13 * i) % min(160, L - last)]
    else:
        step = L // 32
        cols = [i * step, (10 + i) * step, (20 + i) * step + step - 1]
    return sorted(set(cols) | ({0, L - 1} if i == 0 else set()))


def row_hits(rows, L, rng):
    """Every row of `rows` in its own columns."""
    return [(r, c, int(rng.integers(1, 256))) for i, r in enumerate(rows) for c in columns(L, i)]


def filled(rows, n, k, e):
    """`rows` without repeats, then rows from the middle of the data and the
    parity rows, n in all."""
    out = list(dict.fromkeys(rows))
    spare = [r for r in (k // 2, k + e // 2, 1, k + 1, k // 3, k - 2, 0, k + e - 2, 2, 3, 4) if 0 <= r < k + e]
    for r in spare:
        if len(out) >= n:
            break
        if r not in out:
            out.append(r)
    assert len(out) >= n
    return out[:n]


ROUNDS = 2
SINGLES = B - 3
MULTI, OVER, CLEAN = B - 3, B - 2, B - 1


def band_rows(k, e, rnd):
    """What round `rnd` plants, per block the rows: blocks 0 .. B - 4 one of
    gpu_family.band_members each, block B - 3 min(5, e - 1) of them together
    (filled up with other rows where the shape has fewer), block B - 2 more
    rows than min(8, e - 1), which no list length takes, block B - 1 none.  Over
    the two rounds every member is planted in a block of the first two kinds."""
    m = gf.band_members(k, e)
    at = SINGLES * rnd
    rows = [[m[(at + i) % len(m)]] for i in range(SINGLES)]
    n = min(5, e - 1)
    rows.append(sorted(filled([m[(at + SINGLES + i) % len(m)] for i in range(min(n, len(m)))], n, k, e)))
    rows.append(sorted(filled(m[::-1], min(8, e - 1) + 1, k, e)))
    rows.append([])
    return rows


def band_plan(k, e, L, rnd):
    """band_rows as damage: [[(row, column, x)]] per block."""
    rng = np.random.default_rng(4000 * k + 40 * e + rnd + (7 if L != L0 else 0))
    return [row_hits(rows, L, rng) for rows in band_rows(k, e, rnd)]


def cross_pairs(k, e):
    """Pairs of rows of different 64-row bands, one per pair of bands the
    block has, and pairs with rows >= 128 where it has them: [(a, b)], a < b."""
    n = k + e
    bands = range((n + 63) // 64)
    pairs = [(64 * i + 3 + j, min(64 * j + 5 + i, n - 1)) for i in bands for j in bands if i < j]
    if n > 130:
        pairs += [(128, n - 1), (n - 2, n - 1), (2, 129)]
    if k + 1 < n - 1 and (k + 1) // 64 != (n - 1) // 64:
        pairs.append((k + 1, n - 1))  # two parity rows of different bands
    return sorted({p for p in pairs if p[0] < p[1]})


CORRECT_B = 6
PLANNED, BANDS, ONES, THREES = (0, 1), 2, 3, 4


def correct_plan(k, e, L):
    """The correction's damage, CORRECT_B blocks: blocks 0 and 1 as
    correct_generated_cases.plan lays them into the tile; block 2
    correct_cases.band_pairs and cross_pairs, a column each; block 3 single
    rows of every band (one-row corrections at t = 1 and 2); block 4 three
    rows of three bands in a column and three parity rows in another, which
    stay; the last one clean.  At L = 32 the columns are taken modulo."""
    rng = np.random.default_rng(6000 * k + 60 * e + (7 if L != L0 else 0))
    x = lambda: int(rng.integers(1, 256))  # noqa: E731
    out = [[(r, c, v) for _, c, hits in gc.plan(k, e, L, b) for r, v in hits] for b in PLANNED]
    pairs = [[r for r, _ in hits] for _, hits in cc.band_pairs(k, e)] + [list(p) for p in cross_pairs(k, e)]
    at = lambda n: (7 + 233 * n) % L0 if L == L0 else n  # noqa: E731
    assert len(pairs) <= 32 and len({at(n) for n in range(len(pairs))}) == len(pairs)
    out.append([(r, at(n), x()) for n, p in enumerate(pairs) for r in p])
    out.append(row_hits(filled(gf.band_members(k, e), 9, k, e), L, rng))
    n = k + e
    three = [3, min(70, k - 1), n - 1] if k <= 128 else [3, 70, 130]
    out.append([(r, 11, x()) for r in three] + [(r, 17, x()) for r in (k, k + e // 2, n - 1)])
    out.append([])
    assert len(out) == CORRECT_B
    return out, pairs


def degraded_u(e, checked=False):
    return min(7 if checked else 8, e)


# --- the models, on syndromes and on the bad columns ---

def syndromes_of(c, L, hits):
    """The syndromes (e, L) of a consistent block damaged as `hits`: they are
    linear in the rows, so what the block holds does not matter."""
    c = np.asarray(c, np.uint8)
    e, k = c.shape
    syn = np.zeros((e, L), np.uint8)
    for r, col, x in hits:
        if r < k:
            syn[:, col] ^= sm.MUL[c[:, r], x]
        else:
            syn[r - k, col] ^= x
    return syn


def on_bad_columns(model, c, src, par, syn, clean):
    """model(c, src, par) -> (src', par', verdict) run on the columns where
    `syn` is not zero; (verdict, [(row, column, x)] the call XORs in)."""
    bad = np.flatnonzero(syn.any(axis=0))
    if len(bad) == 0:
        return clean, []
    s, p = np.ascontiguousarray(src[:, bad]), np.ascontiguousarray(par[:, bad])
    s2, p2, verdict = model(c, s, p)
    k = s.shape[0]
    fix = [(int(r), int(bad[i]), int(v)) for r, i, v in zip(*np.nonzero(s ^ s2), (s ^ s2)[np.nonzero(s ^ s2)])]
    fix += [(k + int(r), int(bad[i]), int(v)) for r, i, v in zip(*np.nonzero(p ^ p2), (p ^ p2)[np.nonzero(p ^ p2)])]
    return tuple(verdict), fix


def repair_verdict(c, src, par, syn, mode):
    return on_bad_columns(lambda c_, s, p: rm.repair(c_, s, p, mode), c, src, par, syn, (0, 0, rm.CLEAN, -1))


def correct_verdict(c, src, par, syn, t):
    return on_bad_columns(lambda c_, s, p: cm.correct(c_, s, p, t), c, src, par, syn, (0, 0, 0, cm.CLEAN, -1))


def zero_block(k, e, L, hits):
    """The all-zero block, which every linear code holds, damaged as `hits`."""
    src, par = np.zeros((k, L), np.uint8), np.zeros((e, L), np.uint8)
    for r, col, x in hits:
        (src[r] if r < k else par[r - k])[col] ^= x
    return src, par


# --- the seeded draw ---

Case = namedtuple("Case", "seed k e kind L mode tiles call arg blocks")
DRAW_K = [2, 5, 13, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 160, 200]
DRAW_B = 6
SEED_BASE = 0
DRAW_N = int(os.environ.get("RSGPU_FAMILY_FUZZ_N", "40"))


def draw(seed):
    """One case from its seed: the shape, the matrix kind (every one passed as
    the caller's `coef`), the row length and pitch mode, the tiles per
    workgroup of the two-wave wide layouts (0: the library's choice), the call
    with its argument (repair: the mode; locate: u; correct: t; degraded: u)
    and per block the damaged rows, 1 to 3, the last block clean.  A call that
    locates one row per block gets one row in most blocks."""
    r = np.random.default_rng(seed)
    k = int(r.choice(DRAW_K))
    e = int(r.integers(2, min(64, 250 - k) + 1))
    kind = ("rs", "cauchy", "random")[int(r.integers(0, 3))]
    L = 32 * int(r.integers(1, 201))
    mode = ("eq", "plus48")[int(r.integers(0, 2))]
    tiles = int(r.integers(0, 4))
    call = CALLS[int(r.integers(0, len(CALLS)))]
    if e < 3 and call == "correct":
        call = "scrub"  # t = 1 needs e >= 3
    one_row = call in ("scrub", "degraded")
    if call == "repair":
        arg = rm.MODES[int(r.integers(0, 2))] if e >= 3 else "one_row"
        one_row = arg == "one_row"
    elif call == "locate":
        arg = (3, 8)[int(r.integers(0, 2))]
    elif call == "correct":
        arg = 2 if e >= 5 else 1
    else:
        arg = min(4, e)
    blocks = []
    for b in range(DRAW_B - 1):
        n = int(r.choice((1, 1, 1, 1, 2, 3) if one_row else (1, 2, 3)))
        blocks.append(sorted(int(v) for v in r.choice(k + e, n, replace=False)))
    blocks.append([])
    return Case(seed, k, e, kind, L, mode, tiles, call, arg, blocks)


def draw_cases(n=None):
    return [draw(s) for s in range(SEED_BASE, SEED_BASE + (DRAW_N if n is None else n))]


def case_id(c):
    return "s{}-k{}e{}{}-L{}{}-t{}-{}{}".format(c.seed, c.k, c.e, c.kind, c.L, c.mode, c.tiles, c.call, c.arg)


def draw_lists(case):
    """The degraded case's lists: per block 0 to min(u, e - 2) lost rows that
    are not among its damaged ones."""
    r = np.random.default_rng(90000 + case.seed)
    u = case.arg
    lost = np.full((len(case.blocks), u), dm.NONE, np.uint8)
    for b, rows in enumerate(case.blocks):
        n = int(r.integers(0, max(0, min(u, case.e - 2)) + 1))
        free = [v for v in range(case.k + case.e) if v not in rows]
        lost[b] = dm.pad(np.sort(r.choice(free, n, replace=False)), u)
    return lost


def draw_hits(case):
    """The case's damage.  The correction's rows share their columns: one row
    alone, a pair, or three that stay (and a pair beside them); every other
    call's rows have columns of their own."""
    r = np.random.default_rng(80000 + case.seed)
    out = []
    for rows in case.blocks:
        if case.call != "correct":
            out.append(row_hits(rows, case.L, r))
            continue
        hits = []
        for i in range(3):  # columns(L, i) of a row: the same three positions for every i
            for c in columns(case.L, i):
                live = rows if i == 0 else rows[:2] if i == 1 else rows[-1:]
                hits += [(row, c, int(r.integers(1, 256))) for row in live]
        out.append(hits)
    return out


def model_status(case, c, hits, lost=None):
    """The status of every block of a drawn case in its call's model, and the
    value that means DAMAGED there."""
    k, e, L = case.k, case.e, case.L
    out = []
    for b, h in enumerate(hits):
        syn = syndromes_of(c, L, h)
        if case.call == "scrub":
            out.append(sm.report(c, syn)[1])
        elif case.call == "locate":
            out.append(lm.report_syn(c, syn, case.arg)[0][1])
        elif case.call == "degraded":
            out.append(dm.report_syn(c, syn, lost[b])[1])
        else:
            src, par = zero_block(k, e, L, h)
            verdict = repair_verdict(c, src, par, syn, case.arg)[0] if case.call == "repair" else \
                correct_verdict(c, src, par, syn, case.arg)[0]
            out.append(verdict[-2])
    damaged = {"scrub": sm.DAMAGED, "locate": lm.DAMAGED, "degraded": dm.DAMAGED, "repair": rm.DAMAGED,
               "correct": cm.DAMAGED}[case.call]
    return out, damaged
