#!/usr/bin/env python3
"""The repair's measurement (profiles/repair/README.md): fused scrub, repair
COLUMNS and repair ONE_ROW at one shape, in one process on the same buffers.

After one untimed, checked run of each kind: `rounds` mirrored rounds of
scrub, columns, one_row, one_row, columns, scrub on clean data; then the
damaged case, one block in 64 with a 4 KB run of one source row damaged anew
before every run, in both modes.  A run's time is the sum of its kernels'
HIP-event times from rsgpu_timing_read; the kernels' names and times are kept.

    python tools/repair_measure.py out.json [--k 64 --e 32 --len 1000000 --blocks 1024 --rounds 12]

With --kernel generated (profiles/repair_generated/README.md) the same process
measures the generated repair (rsgpu_set_repair_kernel GENERATED) against the
repair it replaces (--against two_pass | fused: the scrub kernel choice under
the repair kernel AUTO) and against the GENERATED scrub with RSGPU_SCRUB_LOCATE,
for any matrix (--matrix rs | cauchy), in both modes, by measure_lib's mirrored
pairs.  Kinds: `generated_scrub` (clean); `{generated,base}_{columns,one_row}`
on clean blocks, `..._one` with data row b mod k of block b bad in 1 % of the
byte columns, `..._whole` with that row bad in every column.  The damage is
XORed in before every damaged run, outside the timed part; the run repairs it.
After one untimed, checked run of each kind (the generated kinds must have run
k_rs_jit_repair and no encode; every damaged block REPAIRED in its row with the
damaged columns counted, and the blocks CLEAN afterwards): `rounds` mirrored
rounds, every kind twice per round; the result keeps every run's total and
per-kernel times, one record per kind.  The summary holds the statistics per kind
with the kernels' medians, generated / base and generated / generated_scrub
over the mirrored pairs (same round, same half), and per kind the A/A ratio of
its own two runs of a round (first half / second half), the spread a pair's
ratio is to be read against.

    python tools/repair_measure.py out.json --kernel generated [--against {two_pass,fused}]
                                            [--matrix {rs,cauchy}] [--k ... --rounds 12]
"""
import numpy as np
import torch

import measure_lib as ml  # puts the engine's directory on the path
import rsgpu  # noqa: E402


def per_kind(runs, kinds):
    """The runs of mirrored_rounds as one record per kind, times in ms to 0.1
    us in the order they ran (round 0 first half, round 0 second half, round 1
    ...): ms the runs' totals, kernels the split of each, pos the kind's two
    places in a round."""
    out = []
    for kind in kinds:
        mine = [r for r in runs if r["kind"] == kind]
        names = sorted({n for r in mine for n in r["kernels"]})
        out.append({"kind": kind, "pos": sorted({r["pos"] for r in mine}), "ms": [round(r["ms"], 4) for r in mine],
                    "kernels": {n: [round(r["kernels"].get(n, 0.0), 4) for r in mine] for n in names}})
    return out


def rounded(v, digits=5):
    """v with every float in it rounded: the summary's ms and ratios to 5 places."""
    if isinstance(v, float):
        return round(v, digits)
    if isinstance(v, dict):
        return {k: rounded(x, digits) for k, x in v.items()}
    return v


def generated(a):
    """--kernel generated: the generated repair against a.against's and against
    the GENERATED scrub."""
    k, e, L, B = a.k, a.e, a.len, a.blocks
    coef = None if a.matrix == "rs" else rsgpu.gf_gen_cauchy1_matrix(k + e, k)[k:]
    ctx, enc = ml.setup(a, coef)
    dev, pitch = enc.src.device, enc.pitch
    srep, rrep = ml.reports(enc), ml.reports(enc, rsgpu.REPAIR_REPORT_DTYPE)
    vs = enc.src.view(B, k, pitch)
    rng = np.random.default_rng(9)
    blk = torch.arange(B, device=dev)
    row = blk % k
    cols = torch.from_numpy(np.sort(rng.choice(L, max(1, L // 100), replace=False))).to(dev)
    x = torch.from_numpy(rng.integers(1, 256, (B, len(cols)), dtype=np.uint8)).to(dev)
    w = torch.from_numpy(rng.integers(1, 256, L, dtype=np.uint8)).to(dev)

    def one():
        vs[blk[:, None], row[:, None], cols[None, :]] ^= x

    def whole():
        vs[blk, row, :L] ^= w[None, :]

    damage = {"one": (one, len(cols)), "whole": (whole, L)}
    torch.cuda.synchronize()

    def run(kind):
        """One timed run: (ms, {kernel name: ms}); a damaged kind is damaged first."""
        if kind == "generated_scrub":
            ctx.set_scrub_kernel("generated")
            try:
                return ml.timed(ctx, lambda: ctx.scrub_blocks(k, e, L, pitch, B, enc.src, enc.par, srep, coef=coef))
            finally:
                ctx.set_scrub_kernel("auto")
        form, mode = kind.split("_", 1)
        hit = next((d for d in damage if mode.endswith("_" + d)), None)
        if hit:
            mode = mode.removesuffix("_" + hit)
            damage[hit][0]()
            torch.cuda.synchronize()
        ctx.set_repair_kernel("generated" if form == "generated" else "auto")
        ctx.set_scrub_kernel(a.against)
        try:
            return ml.timed(ctx, lambda: ctx.repair_blocks(k, e, L, pitch, B, enc.src, enc.par, rrep, coef=coef,
                                                           mode=mode))
        finally:
            ctx.set_repair_kernel("auto")
            ctx.set_scrub_kernel("auto")

    modes = ["columns", "one_row"]
    tails = ["", "_one", "_whole"]
    kinds = ["generated_scrub"] + [f"{form}_{m}{t}" for t in tails for form in ("generated", "base") for m in modes]
    want_base = "k_rs_bs_repair" if a.against == "fused" else "k_repair_compare"
    hrow = row.cpu().numpy()
    for kind in kinds:  # untimed and checked
        srep.fill_(0xA5)
        rrep.fill_(0xA5)
        _, by = run(kind)
        if kind == "generated_scrub":
            assert "k_rs_jit_scrub" in by and ml.all_clean(srep), (kind, sorted(by))
            continue
        if kind.startswith("generated_"):
            assert "k_rs_jit_repair" in by and not any("encode" in n or n == "k_repair_compare" for n in by), \
                (kind, sorted(by))
        else:
            assert want_base in by and "k_rs_jit_repair" not in by, (kind, sorted(by))
        r = rrep.cpu().numpy().view(rsgpu.REPAIR_REPORT_DTYPE)
        hit = next((d for d in damage if kind.endswith("_" + d)), None)
        if not hit:
            assert (r["status"] == rsgpu.REPAIR_CLEAN).all() and (r["repaired_columns"] == 0).all(), kind
        else:
            n = damage[hit][1]
            assert (r["status"] == rsgpu.REPAIR_REPAIRED).all() and (r["row"] == hrow).all(), kind
            assert (r["bad_columns"] == n).all() and (r["repaired_columns"] == n).all(), kind
        ctx.set_scrub_kernel("two_pass")
        ctx.scrub_blocks(k, e, L, pitch, B, enc.src, enc.par, srep, coef=coef)
        ctx.set_scrub_kernel("auto")
        torch.cuda.synchronize()
        assert ml.all_clean(srep), (kind, "the blocks after the repair")

    out = {**ml.header(enc), "matrix": a.matrix, "against": a.against, "bad_columns_one": int(len(cols))}
    runs = ml.mirrored_rounds(kinds, a.rounds, run)
    out["runs"] = per_kind(runs, kinds)
    summ = ml.summarise(runs, kinds, kernel_medians=True)
    half = len(kinds)
    at = {(r["round"], r["pos"] >= half, r["kind"]): r["ms"] for r in runs}
    pairs = [(rnd, h) for rnd in range(a.rounds) for h in (False, True)]
    for kind in kinds:
        summ[kind]["aa_first_over_second"] = ml.stats([at[(rnd, False, kind)] / at[(rnd, True, kind)]
                                                       for rnd in range(a.rounds)])
    for t in tails:
        for m in modes:
            g, b = f"generated_{m}{t}", f"base_{m}{t}"
            summ[g]["over_base_in_pairs"] = ml.stats([at[(rnd, h, g)] / at[(rnd, h, b)] for rnd, h in pairs])
            summ[g]["over_base"] = summ[g]["median"] / summ[b]["median"]
    for m in modes:
        g = f"generated_{m}"
        summ[g]["over_scrub_in_pairs"] = ml.stats([at[(rnd, h, g)] / at[(rnd, h, "generated_scrub")]
                                                   for rnd, h in pairs])
    ml.finish(a.out, out, rounded(summ))
    ctx.close()


def main():
    ap = ml.shape_parser()
    ap.add_argument("--damaged-runs", type=int, default=6)
    ap.add_argument("--kernel", choices=["fused", "generated"], default="fused")
    ap.add_argument("--against", choices=["two_pass", "fused"], default="two_pass")
    ap.add_argument("--matrix", choices=["rs", "cauchy"], default="rs")
    a = ap.parse_args()
    if a.kernel == "generated":
        return generated(a)
    k, e, L, B = a.k, a.e, a.len, a.blocks

    ctx, enc = ml.setup(a)
    ctx.set_scrub_kernel("fused")
    srep, rrep = ml.reports(enc), ml.reports(enc, rsgpu.REPAIR_REPORT_DTYPE)
    torch.cuda.synchronize()

    def run(kind):
        """One timed call: (total ms, {kernel name: ms}), the reports left in srep / rrep."""
        if kind == "scrub":
            return ml.timed(ctx, lambda: ctx.scrub_blocks(k, e, L, enc.pitch, B, enc.src, enc.par, srep))
        return ml.timed(ctx, lambda: ctx.repair_blocks(k, e, L, enc.pitch, B, enc.src, enc.par, rrep, mode=kind))

    def scrub_reports():
        return srep.cpu().numpy().view(rsgpu.SCRUB_REPORT_DTYPE)

    def repair_reports():
        return rrep.cpu().numpy().view(rsgpu.REPAIR_REPORT_DTYPE)

    # untimed and checked: clean data, every block CLEAN
    run("scrub")
    assert (scrub_reports()["status"] == rsgpu.SCRUB_CLEAN).all()
    for mode in ("columns", "one_row"):
        run(mode)
        r = repair_reports()
        assert (r["status"] == rsgpu.REPAIR_CLEAN).all() and (r["repaired_columns"] == 0).all()

    kinds = ["scrub", "columns", "one_row"]
    out = {**ml.header(enc), "clean": ml.mirrored_rounds(kinds, a.rounds, run), "damaged": []}

    # damaged: one block in 64, bytes [8192, 12288) of source row 3
    hit = list(range(5, B, 64))
    rows = enc.src.view(B, k, enc.pitch)

    def damage():
        rows[hit, 3, 8192:12288] ^= 0x5A
        torch.cuda.synchronize()

    damage()
    run("scrub")  # untimed: the scrub names the row
    s = scrub_reports()
    assert (s["status"][hit] == rsgpu.SCRUB_ONE_ROW).all() and (s["row"][hit] == 3).all()
    assert int((s["status"] != rsgpu.SCRUB_CLEAN).sum()) == len(hit)
    first = True
    for n in range(a.damaged_runs):
        for mode in ("columns", "one_row"):
            if not first:
                damage()
            first = False
            ms, by = run(mode)
            r = repair_reports()
            assert (r["status"][hit] == rsgpu.REPAIR_REPAIRED).all() and (r["row"][hit] == 3).all()
            assert (r["repaired_columns"][hit] == 4096).all() and int(r["bad_columns"].sum()) == 4096 * len(hit)
            out["damaged"].append({"run": n, "kind": mode, "ms": ms, "kernels": by,
                                   "damaged_blocks": len(hit), "bytes_per_block": 4096})
            run("scrub")
            assert (scrub_reports()["status"] == rsgpu.SCRUB_CLEAN).all()

    summ = ml.summarise(out["clean"], kinds)
    per_round = []
    for rnd in range(a.rounds):
        t = {kd: [r["ms"] for r in out["clean"] if r["round"] == rnd and r["kind"] == kd] for kd in kinds}
        sc = sum(t["scrub"]) / 2
        per_round.append({"round": rnd, "scrub_spread": abs(t["scrub"][0] - t["scrub"][1]) / sc,
                          "columns_over_scrub": sum(t["columns"]) / 2 / sc,
                          "one_row_over_scrub": sum(t["one_row"]) / 2 / sc,
                          "one_row_minus_scrub_ms": sum(t["one_row"]) / 2 - sc})
    summ["per_round"] = per_round
    for mode in ("columns", "one_row"):
        summ["damaged_" + mode] = ml.stats([r["ms"] for r in out["damaged"] if r["kind"] == mode])
    gated = [r["kernels"].get("k_rs_bs_repair_gated", 0.0) for r in out["clean"] if r["kind"] == "one_row"]
    summ["one_row_gated_launch_clean"] = ml.stats(gated)
    ml.finish(a.out, out, summ)
    ctx.close()


if __name__ == "__main__":
    main()
