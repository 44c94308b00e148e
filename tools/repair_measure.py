#!/usr/bin/env python3
"""The repair's measurement (profiles/repair/README.md): fused scrub, repair
COLUMNS and repair ONE_ROW at one shape, in one process on the same buffers.

After one untimed, checked run of each kind: `rounds` mirrored rounds of
scrub, columns, one_row, one_row, columns, scrub on clean data; then the
damaged case, one block in 64 with a 4 KB run of one source row damaged anew
before every run, in both modes.  A run's time is the sum of its kernels'
HIP-event times from rsgpu_timing_read; the kernels' names and times are kept.

    python tools/repair_measure.py out.json [--k 64 --e 32 --len 1000000 --blocks 1024 --rounds 12]
"""
import torch

import measure_lib as ml  # puts the engine's directory on the path
import rsgpu  # noqa: E402


def main():
    ap = ml.shape_parser()
    ap.add_argument("--damaged-runs", type=int, default=6)
    a = ap.parse_args()
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
