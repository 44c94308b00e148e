"""The cases of tests/test_gpu_family_generated_wide.py on the models alone
(tests/family_wide_cases.py): the damage the GPU suite plants at wide k and
wide e is located, listed and corrected by the numpy models, so that the
device comparison is not one of DAMAGED with DAMAGED; every row around the
64-row bands is planted; the seeded draw reaches every layout and every call;
and the host's choice between the generated correction and TWO_PASS at the
four-wave 16-row layout's LDS budget (csrc/rs_jit.hip jit_correct_fits) is
where the suite expects it."""
import ctypes as C

import numpy as np
import pytest

import correct_fused_cases as fc
import correct_generated_cases as gc
import correct_model as cm
import degraded_model as dm
import family_wide_cases as fw
import gpu_family as gf
import locate_model as lm
import repair_model as rm
import rsgpu
import scrub_model as sm

N = dm.NONE
LOCATED = (lm.ONE_ROW, lm.ROWS)


def test_shapes_reach_every_layout_and_every_matrix_is_locatable():
    assert {fw.layout(e) for _, e, _ in fw.SHAPES} == set(fw.LAYOUTS)
    chunk = {8: 8, 10: 5, 12: 6, 16: 6}
    for k, e, kind in fw.SHAPES:
        assert k > 64 and k + e <= 250 and sm.locatable(fw.matrix(k, e, kind)), (k, e)
        if (k, e) not in ((100, 20), (186, 64)):  # the C5 code; k + e = 250 at e = 64
            assert k % chunk[fw.layout(e)[1]], (k, e)
    assert all(s in fw.SHAPES and fw.layout(s[1])[0] == 2 for s in fw.TILED)
    assert {fw.layout(e)[1] for _, e, _ in fw.TILED} == {10, 12, 16}
    for c in (fw.columns(fw.L0, i) for i in range(10)):
        assert {v // fw.TILE for v in c} >= {0, 3} and len({v // fw.TILE for v in c}) >= 3
    for L in (32, 64, 2112, fw.L0, 6400):
        cols = [v for i in range(10) for v in fw.columns(L, i)]
        assert len(cols) == len(set(cols)) and min(cols) == 0 and max(cols) == L - 1


def test_the_correction_s_tables_fit_up_to_the_line():
    """jit_correct_fits(k, e, 2) on the host: (151, 64) and (183, 60) inside the
    chunk buffers, (152, 64) and (184, 60) not; every other shape of the suite
    inside, and t = 1 everywhere."""
    f = rsgpu.testhooks().rsgpu_internal_jit_correct_fits
    f.restype, f.argtypes = C.c_int, [C.c_int, C.c_int, C.c_int]
    assert [f(151, 64, 2), f(152, 64, 2), f(183, 60, 2), f(184, 60, 2)] == [1, 0, 1, 0]
    assert [(k, e) for k, e, _ in fw.SHAPES if not f(k, e, 2)] == fw.NO_FIT
    assert all(f(k, e, 1) == 1 for k, e, _ in fw.SHAPES)
    # the line is 256 e + 32 k <= 21240 from e = 49 to 64, and nowhere below
    for e in range(5, 65):
        for k in range(1, 251 - e):
            assert f(k, e, 2) == fw.fits(k, e) == (e <= 48 or 256 * e + 32 * k <= 21240), (k, e)
    assert f(0, 64, 2) == f(187, 64, 2) == f(10, 65, 2) == f(10, 5, 3) == -1


@pytest.mark.parametrize("L", fw.LENGTHS)
@pytest.mark.parametrize("k,e,kind", fw.SHAPES, ids=str)
def test_rows_around_the_bands_are_located(k, e, kind, L):
    """Scrub, repair and locate on the two rounds of band_plan: a block of one
    row is ONE_ROW with that row and REPAIRED in both modes; a block of n <=
    min(u, e - 1) rows lists them (Cauchy; gf_gen_rs_matrix: three quarters of
    them located); more rows than that are DAMAGED; COLUMNS repairs every
    column of every block; over the rounds every band member is planted in a
    block that is located."""
    c = fw.matrix(k, e, kind)
    seen, within, located = set(), 0, 0
    for rnd in range(fw.ROUNDS):
        rows, plan = fw.band_rows(k, e, rnd), fw.band_plan(k, e, L, rnd)
        assert len(plan) == fw.B and not plan[fw.CLEAN] and len(rows[fw.OVER]) > min(max(fw.US), e - 1)
        for b, hits in enumerate(plan):
            cols = {col for _, col, _ in hits}
            assert len(cols) == len(hits) and all(0 <= col < L for col in cols)
            if L == fw.L0 and hits:
                assert {col // fw.TILE for col in cols} >= {0, 3} and cols & {fw.TILE + i for i in range(2 * fw.TILE)}
            syn = fw.syndromes_of(c, L, hits)
            src, par = fw.zero_block(k, e, L, hits)
            scrub = sm.report(c, syn)
            one_row, fix1 = fw.repair_verdict(c, src, par, syn, "one_row")
            columns, fix = fw.repair_verdict(c, src, par, syn, "columns")
            n = len(rows[b])
            if n == 0:
                assert scrub == (0, sm.CLEAN, -1) and not fix
            elif n == 1:
                assert scrub == (len(hits), sm.ONE_ROW, rows[b][0])
                assert one_row == columns == (len(hits), len(hits), rm.REPAIRED, rows[b][0])
                assert sorted(fix1) == sorted(fix) == sorted(hits)
            else:
                assert scrub == (len(hits), sm.DAMAGED, -1) and one_row == (len(hits), 0, rm.DAMAGED, -1) and not fix1
                assert columns == (len(hits), len(hits), rm.REPAIRED, -1) and sorted(fix) == sorted(hits)
            for u in fw.US:
                rep, lst = lm.report_syn(c, syn, u)
                if 1 <= n <= min(u, e - 1):
                    within += 1
                    located += rep[1] in LOCATED
                    if rep[1] in LOCATED:
                        seen.update(rows[b])
                    if kind == "cauchy":
                        assert rep == (len(hits), lm.ONE_ROW if n == 1 else lm.ROWS, rows[b][0]), (rnd, b, u)
                        assert list(lst) == rows[b] + [N] * (u - n)
                elif n:
                    assert rep == (len(hits), lm.DAMAGED, -1), (rnd, b, u, rep)
    assert seen >= set(gf.band_members(k, e)), (seen, gf.band_members(k, e))
    assert 4 * located >= 3 * within, (located, within)
    if k + e > 129:
        assert any(r >= 128 for r in seen)


def test_rows_from_128_on_occur():
    wide = [(k, e) for k, e, _ in fw.SHAPES if any(r >= 128 for r in gf.band_members(k, e))]
    assert len(wide) >= 8 and {fw.layout(e) for _, e in wide} >= {(2, 16), (4, 10), (4, 16)}


@pytest.mark.parametrize("k,e,kind", fw.SHAPES, ids=str)
def test_the_correction_s_plan(k, e, kind):
    """correct_plan at L0 on the model: every pair column of the band block
    is a two-row correction with the planted rows and values (Cauchy; three
    quarters of them with gf_gen_rs_matrix), the pairs reach across the bands
    and, where the block has them, rows >= 128; the tile-planned blocks hold
    at least 9 two-row corrections, a one-row one and a column left alone; the
    block of single rows is REPAIRED at t = 1; the three-row columns stay."""
    c = fw.matrix(k, e, kind)
    L = fw.L0
    plan, pairs = fw.correct_plan(k, e, L)
    assert any(a // 64 != b // 64 for a, b in pairs) and all(a < b for a, b in pairs)
    if k + e > 130:
        assert any(b >= 128 for _, b in pairs) and any(a >= 128 for a, _ in pairs)
    two = 0
    by_col = {}
    for r, col, x in plan[fw.BANDS]:
        by_col.setdefault(col, []).append((r, x))
    assert len(by_col) == len(pairs)
    for col, hits in by_col.items():
        fix = cm.verdict(c, fw.syndromes_of(c, 1, [(r, 0, x) for r, x in hits])[:, 0], 2)
        two += sorted(fix) == sorted(hits)
        assert kind != "cauchy" or sorted(fix) == sorted(hits), (col, hits, fix)
    assert 4 * two >= 3 * len(pairs)
    for b in fw.PLANNED:
        kinds = {kd for kd, _, _ in gc.plan(k, e, L, b)}
        assert set(fc.PAIR_KINDS) | {"one", "one-parity", "three", "three-mixed"} <= kinds
        syn = fw.syndromes_of(c, L, plan[b])
        verdict, _ = fw.correct_verdict(c, *fw.zero_block(k, e, L, plan[b]), syn, 2)
        assert verdict[2] >= 9 and verdict[1] > verdict[2] and verdict[0] > verdict[1] and verdict[3] == cm.PARTIAL
    for t in (1, 2):
        hits = plan[fw.ONES]
        verdict, fix = fw.correct_verdict(c, *fw.zero_block(k, e, L, hits), fw.syndromes_of(c, L, hits), t)
        assert verdict == (len(hits), len(hits), 0, cm.REPAIRED, -1) and sorted(fix) == sorted(hits)
    hits = plan[fw.THREES]
    verdict, fix = fw.correct_verdict(c, *fw.zero_block(k, e, L, hits), fw.syndromes_of(c, L, hits), 2)
    assert kind != "cauchy" or (verdict == (2, 0, 0, cm.DAMAGED, -1) and not fix)
    assert not plan[-1]


@pytest.mark.parametrize("k,e,kind", fw.SHAPES, ids=str)
def test_the_degraded_lists_and_damage(k, e, kind):
    """gpu_family.wide_lists and wide_plan at B blocks: every band member is
    in a list; the ONE_ROW block names the last data row, the other one is
    DAMAGED, on the degraded model, for the scrub's lists (u = min(8, e)) and
    the checked rebuild's (u = 7)."""
    c = fw.matrix(k, e, kind)
    for u in (fw.degraded_u(e), fw.degraded_u(e, True)):
        lost = gf.wide_lists(k, e, u, fw.B)
        assert {int(r) for r in lost.ravel()} - {N} >= set(gf.band_members(k, e))
        hits, one, two = gf.wide_plan(lost, k, e, fw.L0)
        for b in range(fw.B):
            syn = fw.syndromes_of(c, fw.L0, [(r, col, x) for blk, r, col, x in hits if blk == b])
            rep = dm.report_syn(c, syn, lost[b])
            want = (1, dm.ONE_ROW, gf.wide_row(k, e)) if b == one else (2, dm.DAMAGED, -1) if b == two else \
                (0, dm.UNCHECKED if len(dm.list_rows(lost[b], k, e)) == e else dm.CLEAN, -1)
            assert rep == want, (u, b, rep)
        assert gf.wide_row(k, e) >= 64


def test_the_draw_reaches_every_layout_and_every_call():
    """The default 40 cases: every layout of the generated kernels, k > 64 on
    a two-wave and on a four-wave one, each call at least four times, every
    matrix locatable, and on the models at most a quarter of the damaged
    blocks DAMAGED."""
    cases = fw.draw_cases(40)
    assert cases == fw.draw_cases(40) and len({fw.case_id(c) for c in cases}) == 40
    assert {fw.layout(c.e) for c in cases} == set(fw.LAYOUTS)
    assert any(c.k > 64 and fw.layout(c.e)[0] == 2 for c in cases)
    assert any(c.k > 64 and fw.layout(c.e)[0] == 4 for c in cases)
    assert all(sum(c.call == call for c in cases) >= 4 for call in fw.CALLS)
    assert {c.kind for c in cases} == {"rs", "cauchy", "random"} and {c.mode for c in cases} == {"eq", "plus48"}
    assert {c.tiles for c in cases if fw.layout(c.e) in ((2, 10), (2, 12), (2, 16))} >= {2, 3}
    blocks = damaged = 0
    for case in cases:
        assert case.k in fw.DRAW_K and 2 <= case.e <= min(64, 250 - case.k) and case.L % 32 == 0 and 32 <= case.L <= 6400
        assert all(1 <= len(rows) <= 3 for rows in case.blocks[:-1]) and not case.blocks[-1]
        c = fw.matrix(case.k, case.e, case.kind, case.seed)
        assert c.shape == (case.e, case.k) and sm.locatable(c)
        hits = fw.draw_hits(case)
        lost = fw.draw_lists(case) if case.call == "degraded" else None
        if lost is not None:
            assert all(dm.list_rows(lst, case.k, case.e) is not None for lst in lost)
            assert not any(set(dm.list_rows(lst, case.k, case.e)) & set(rows) for lst, rows in zip(lost, case.blocks))
        status, bad = fw.model_status(case, c, hits, lost)
        assert status[-1] == 0  # CLEAN in every model
        blocks += len(status) - 1
        damaged += sum(s == bad for s in status[:-1])
    assert 4 * damaged <= blocks, (damaged, blocks)
