#!/usr/bin/env python3
"""The measurement of the correction per column (profiles/correct/README.md):
rsgpu_correct_blocks against rsgpu_repair_blocks in COLUMNS mode under the
TWO_PASS scrub kernel on the same blocks, clean and with four kinds of damage,
and the TWO_PASS locate followed by the rebuild on three of them, at one shape,
in one process on the same buffers.

Kinds: `columns_clean` (rsgpu_repair_blocks, COLUMNS, TWO_PASS) and
`correct_clean` (t = 2) on consistent blocks; `correct1_one` and `correct_one`
(t = 1 and t = 2; one data row per block, b mod k, bad in 1 % of the byte
columns); `correct_two` (a second data row bad in the same columns);
`correct_whole` (two whole data rows per block bad: every column takes the
pair search); `correct_scattered` (12 data rows per block, each pair of them
bad in a sixth of those 1 % of the columns: at most two rows per column);
`heal_one`, `heal_two`, `heal_whole`: rsgpu_locate_blocks (TWO_PASS) and
rsgpu_rebuild_blocks of its lists on the damage of the first three.  Damage is
XORed into the rows before every run, outside the timed part; every kind
brings the rows back, which an untimed, checked run of each kind and a scrub at
the end confirm.  Then `rounds` mirrored rounds, every kind twice per round.  A
run's time is the sum of its kernels' HIP-event times from rsgpu_timing_read.

With --fused the fused forms are measured beside them
(profiles/correct_fused/README.md): `fused_correct_*` is rsgpu_correct_blocks
under rsgpu_set_correct_kernel FUSED (k_rs_bs_correct) on the same kinds of
damage, `fused_columns_clean` is rsgpu_repair_blocks COLUMNS under the FUSED
scrub kernel (k_rs_bs_repair), the yardstick of `fused_correct_clean`; the
summary holds that ratio over the mirrored pairs as well.  The kinds of a run
are then the fused ones and `correct_clean`; --kinds names others.

With --generated the form fused into the generated scrub is measured
(profiles/correct_generated/README.md), for a named matrix (--matrix rs |
cauchy: gf_gen_rs_matrix passed as `coef`, so that a compiled code such as
(64, 32) does not take the compiled form, or gf_gen_cauchy1_matrix):
`gen_correct_*` is rsgpu_correct_blocks under rsgpu_set_correct_kernel FUSED
with the scrub kernel GENERATED (k_rs_jit_correct) on the same kinds of damage,
`gen_columns_clean` is rsgpu_repair_blocks COLUMNS under
rsgpu_set_repair_kernel GENERATED (k_rs_jit_repair), the yardstick of
`gen_correct_clean`; every kind of damage also runs under TWO_PASS, and the
summary holds gen_correct_clean / gen_columns_clean, that yardstick's own
first-over-second-half spread, and generated / TWO_PASS per kind, all over the
mirrored pairs.  With --fused as well (the compiled codes, --matrix rs)
`fused_correct_clean` runs beside them without `coef`.

Besides the statistics per kind the summary holds correct_clean /
columns_clean over the mirrored pairs (same round, same half), to be read
against the two kinds' own run-to-run spread.

    python tools/correct_measure.py out.json [--k 64 --e 32 --len 1000000 --blocks 1024 --rounds 12]
                                             [--skip kind,kind] [--fused] [--kinds kind,kind]
                                             [--generated] [--matrix {rs,cauchy}]
"""
import sys

import numpy as np
import torch

import measure_lib as ml  # puts the engine's directory on the path
import rsgpu  # noqa: E402

DT = rsgpu.CORRECT_REPORT_DTYPE
U = rsgpu.LOCATE_MAX_ROWS
SCATTER = 12


def main():
    ap = ml.shape_parser()
    ap.add_argument("--skip", default="", help="kinds to leave out, comma separated")
    ap.add_argument("--fused", action="store_true", help="the fused kinds and correct_clean")
    ap.add_argument("--kinds", default="", help="exactly these kinds, comma separated")
    ap.add_argument("--generated", action="store_true", help="the generated kinds and their TWO_PASS twins")
    ap.add_argument("--matrix", choices=["rs", "cauchy"], default="rs", help="with --generated: the matrix, as coef")
    a = ap.parse_args()
    k, e, L, B = a.k, a.e, a.len, a.blocks
    assert k >= SCATTER and 5 <= e <= 64
    # --generated: the matrix always as `coef`; the compiled kinds pass none
    coef = None
    if a.generated:
        coef = rsgpu.gf_gen_rs_matrix(k + e, k)[k:] if a.matrix == "rs" else rsgpu.gf_gen_cauchy1_matrix(k + e, k)[k:]
    ctx, enc = ml.setup(a, coef)
    ctx.set_scrub_kernel("two_pass")
    ctx.set_locate_kernel("two_pass")
    dev, pitch = enc.src.device, enc.pitch
    crep, rrep, srep = ml.reports(enc, DT), ml.reports(enc, rsgpu.REPAIR_REPORT_DTYPE), ml.reports(enc)
    srep2 = ml.reports(enc)
    lists = torch.empty(B * U, dtype=torch.uint8, device=dev)
    vs = enc.src.view(B, k, pitch)
    rng = np.random.default_rng(9)
    blk = torch.arange(B, device=dev)
    r1 = torch.arange(B, device=dev) % k
    r2 = (r1 + 1 + torch.from_numpy(rng.integers(0, k - 1, B)).to(dev)) % k  # != r1
    ncols = max(SCATTER // 2, L // 100 // (SCATTER // 2) * (SCATTER // 2))
    c1 = torch.from_numpy(np.sort(rng.choice(L, ncols, replace=False))).to(dev)
    x1 = torch.from_numpy(rng.integers(1, 256, (B, ncols), dtype=np.uint8)).to(dev)
    x2 = torch.from_numpy(rng.integers(1, 256, (B, ncols), dtype=np.uint8)).to(dev)
    w1 = torch.from_numpy(rng.integers(1, 256, L, dtype=np.uint8)).to(dev)
    w2 = torch.from_numpy(rng.integers(1, 256, L, dtype=np.uint8)).to(dev)
    # scattered: rows r1 + j (k // 12), j < 12, distinct; the columns in six
    # parts, part m damaged in rows 2 m and 2 m + 1
    part = ncols // (SCATTER // 2)
    srows = [(r1 + j * (k // SCATTER)) % k for j in range(SCATTER)]

    def sparse(rows, c, x):
        vs[blk[:, None], rows[:, None], c[None, :]] ^= x

    def whole(rows, w):
        vs[blk, rows, :L] ^= w[None, :]

    def scattered():
        for j in range(SCATTER):
            m = j // 2
            sel = slice(m * part, (m + 1) * part)
            sparse(srows[j], c1[sel], (x1 if j % 2 == 0 else x2)[:, sel])

    one = lambda: sparse(r1, c1, x1)  # noqa: E731
    two = lambda: (sparse(r1, c1, x1), sparse(r2, c1, x2))  # noqa: E731
    both = lambda: (whole(r1, w1), whole(r2, w2))  # noqa: E731
    FUSED, GEN = "fused_", "gen_"
    damage = {"correct1_one": one, "correct_one": one, "correct_two": two, "correct_whole": both,
              "correct_scattered": scattered, "heal_one": one, "heal_two": two, "heal_whole": both}
    torch.cuda.synchronize()

    def run(kind):
        """One timed run: (ms, {kernel name: ms})."""
        fused, gen = kind.startswith(FUSED), kind.startswith(GEN)
        kind = kind[len(FUSED):] if fused else kind[len(GEN):] if gen else kind
        ctx.set_scrub_kernel("fused" if fused else "generated" if gen else "two_pass")
        ctx.set_correct_kernel("fused" if fused or gen else "two_pass")
        ctx.set_repair_kernel("generated" if gen else "auto")
        c = None if fused else coef
        if kind in damage:
            damage[kind]()
            torch.cuda.synchronize()
        if kind == "columns_clean":
            return ml.timed(ctx, lambda: ctx.repair_blocks(k, e, L, pitch, B, enc.src, enc.par, rrep, coef=c,
                                                           mode="columns"))
        if kind.startswith("heal"):
            def heal():
                ctx.locate_blocks(k, e, L, pitch, B, enc.src, enc.par, U, lists, srep, coef=c)
                ctx.rebuild_blocks(k, e, L, pitch, B, enc.src, enc.par, U, lists, srep2, coef=c, check=False)
            return ml.timed(ctx, heal)
        t = 1 if kind.startswith("correct1") else 2
        return ml.timed(ctx, lambda: ctx.correct_blocks(k, e, L, pitch, B, enc.src, enc.par, crep, coef=c, t=t))

    skip = set(filter(None, a.skip.split(",")))
    every = ["columns_clean", "correct_clean", "correct1_one", "correct_one", "correct_two",
             "correct_whole", "correct_scattered", "heal_one", "heal_two", "heal_whole"]
    if a.fused:
        every = [FUSED + "columns_clean", FUSED + "correct_clean", "correct_clean", FUSED + "correct_one",
                 FUSED + "correct_two", FUSED + "correct_scattered", FUSED + "correct_whole"]
    DAMAGED = ["correct_one", "correct_two", "correct_scattered", "correct_whole"]
    if a.generated:
        every = [GEN + "columns_clean", GEN + "correct_clean", "correct_clean"]
        every += [FUSED + "correct_clean"] if a.fused else []
        every += [kd for d in DAMAGED for kd in (GEN + d, d)]
    if a.kinds:
        every = a.kinds.split(",")
    kinds = [kd for kd in every if kd not in skip]
    bad = {"correct1_one": (ncols, 0), "correct_one": (ncols, 0), "correct_two": (ncols, ncols),
           "correct_whole": (L, L), "correct_scattered": (part * (SCATTER // 2), part * (SCATTER // 2))}
    kernels_seen = {}
    for kind in kinds:  # untimed and checked
        crep.fill_(0xA5)
        ms, by = run(kind)
        print(f"checked {kind}: {ms:.2f} ms", file=sys.stderr, flush=True)
        kernels_seen[kind] = sorted(by)
        fused, gen = kind.startswith(FUSED), kind.startswith(GEN)
        kind = kind[len(FUSED):] if fused else kind[len(GEN):] if gen else kind
        if kind == "columns_clean":
            r = rrep.cpu().numpy().view(rsgpu.REPAIR_REPORT_DTYPE)
            assert (r["status"] == rsgpu.REPAIR_CLEAN).all(), kind
            if gen:
                assert sorted(by) == ["k_repair_finalise", "k_rs_jit_repair"], by
            else:
                assert sorted(by) == ["k_repair_finalise", "k_rs_bs_repair"] if fused else "k_repair_compare" in by, by
        elif kind.startswith("heal"):
            r = srep.cpu().numpy().view(rsgpu.SCRUB_REPORT_DTYPE)
            assert (r["status"] == (rsgpu.SCRUB_ONE_ROW if kind == "heal_one" else rsgpu.SCRUB_ROWS)).all(), kind
        else:
            r = crep.cpu().numpy().view(DT)
            if fused or gen:
                assert sorted(by) == ["k_correct_finalise", "k_rs_bs_correct" if fused else "k_rs_jit_correct"], by
            else:
                assert "k_correct_compare" in by, kind
            if kind == "correct_clean":
                assert (r["status"] == rsgpu.REPAIR_CLEAN).all() and (r["bad_columns"] == 0).all(), kind
            else:
                n, n2 = bad[kind]
                assert (r["status"] == rsgpu.REPAIR_REPAIRED).all() and (r["bad_columns"] == n).all(), kind
                assert (r["corrected_columns"] == n).all() and (r["two_row_columns"] == n2).all(), kind
        ctx.set_scrub_kernel("two_pass")
        ctx.scrub_blocks(k, e, L, pitch, B, enc.src, enc.par, srep, coef=coef)
        torch.cuda.synchronize()
        assert ml.all_clean(srep), "the blocks after " + kind
        bad[FUSED + kind] = bad[GEN + kind] = bad.get(kind, (0, 0))

    def progress(kind):
        out = run(kind)
        print(f"{kind} {out[0]:.2f}", file=sys.stderr, flush=True)
        return out

    out = {**ml.header(enc), "kernels": kernels_seen, "bad_columns": {kd: v[0] for kd, v in bad.items()},
           "runs": ml.mirrored_rounds(kinds, a.rounds, progress)}
    ctx.set_scrub_kernel("two_pass")
    ctx.scrub_blocks(k, e, L, pitch, B, enc.src, enc.par, srep, coef=coef)
    torch.cuda.synchronize()
    assert ml.all_clean(srep), "the blocks after the last run"
    summ = ml.summarise(out["runs"], kinds, kernel_medians=True)
    half = len(kinds)
    at = {(r["round"], r["pos"] >= half, r["kind"]): r["ms"] for r in out["runs"]}
    if "columns_clean" in kinds and "correct_clean" in kinds:
        ratios = [at[(rnd, h, "correct_clean")] / at[(rnd, h, "columns_clean")] for rnd in range(a.rounds)
                  for h in (False, True)]
        summ["correct_clean"]["over_columns_in_pairs"] = ml.stats(ratios)
        summ["correct_clean"]["over_columns_in_pairs"]["mean"] = float(np.mean(ratios))
        cmp_ratios = [r["kernels"]["k_correct_compare"] for r in out["runs"] if r["kind"] == "correct_clean"]
        rep_ratios = [r["kernels"]["k_repair_compare"] for r in out["runs"] if r["kind"] == "columns_clean"]
        summ["correct_clean"]["compare_kernel_over_columns"] = float(np.median(cmp_ratios) / np.median(rep_ratios))
    fc, fr = FUSED + "correct_clean", FUSED + "columns_clean"
    if fc in kinds and fr in kinds:
        ratios = [at[(rnd, h, fc)] / at[(rnd, h, fr)] for rnd in range(a.rounds) for h in (False, True)]
        summ[fc]["over_fused_columns_in_pairs"] = ml.stats(ratios)
        summ[fc]["over_fused_columns_in_pairs"]["mean"] = float(np.mean(ratios))
        # the pairs' own run-to-run spread: each kind's two runs of a round against each other
        for kd in (fc, fr):
            own = [at[(rnd, False, kd)] / at[(rnd, True, kd)] for rnd in range(a.rounds)]
            summ[kd]["first_over_second_half"] = {**ml.stats(own), "mean": float(np.mean(own))}
        if "correct_clean" in kinds:
            summ[fc]["over_two_pass_median"] = summ[fc]["median"] / summ["correct_clean"]["median"]
    gc, gr = GEN + "correct_clean", GEN + "columns_clean"
    if gc in kinds and gr in kinds:
        ratios = [at[(rnd, h, gc)] / at[(rnd, h, gr)] for rnd in range(a.rounds) for h in (False, True)]
        summ[gc]["over_generated_columns_in_pairs"] = {**ml.stats(ratios), "mean": float(np.mean(ratios))}
        for kd in (gc, gr):  # the A/A of each: its two runs of a round against each other
            own = [at[(rnd, False, kd)] / at[(rnd, True, kd)] for rnd in range(a.rounds)]
            summ[kd]["first_over_second_half"] = {**ml.stats(own), "mean": float(np.mean(own))}
    for kd in kinds:  # generated over TWO_PASS (and over the compiled form) in the mirrored pairs
        if kd.startswith(GEN) and kd[len(GEN):] in kinds and kd != gr:
            ratios = [at[(rnd, h, kd)] / at[(rnd, h, kd[len(GEN):])] for rnd in range(a.rounds) for h in (False, True)]
            summ[kd]["over_two_pass_in_pairs"] = {**ml.stats(ratios), "mean": float(np.mean(ratios))}
    if gc in kinds and fc in kinds:
        ratios = [at[(rnd, h, gc)] / at[(rnd, h, fc)] for rnd in range(a.rounds) for h in (False, True)]
        summ[gc]["over_compiled_in_pairs"] = {**ml.stats(ratios), "mean": float(np.mean(ratios))}
    ml.finish(a.out, out, summ)
    ctx.set_repair_kernel("auto")
    ctx.set_correct_kernel("auto")
    ctx.set_scrub_kernel("auto")
    ctx.set_locate_kernel("auto")
    ctx.close()


if __name__ == "__main__":
    main()
