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
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "storage-benchmarks_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rsgpu  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--e", type=int, default=32)
    ap.add_argument("--len", type=int, default=1000000)
    ap.add_argument("--blocks", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--damaged-runs", type=int, default=6)
    a = ap.parse_args()
    k, e, L, B = a.k, a.e, a.len, a.blocks

    ctx = rsgpu.Context(0)
    ctx.set_torch_stream()
    ctx.set_scrub_kernel("fused")
    enc = rsgpu.GpuEncoder(k, L, e, blocks=B, seed=5, ctx=ctx)
    enc.encode_all()
    dev = enc.src.device
    srep = torch.empty(B * rsgpu.SCRUB_REPORT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    rrep = torch.empty(B * rsgpu.REPAIR_REPORT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def run(kind):
        """One timed call: (total ms, {kernel name: ms}), the reports left in srep / rrep."""
        ctx.timing_enable(True)
        try:
            if kind == "scrub":
                ctx.scrub_blocks(k, e, L, enc.pitch, B, enc.src, enc.par, srep)
            else:
                ctx.repair_blocks(k, e, L, enc.pitch, B, enc.src, enc.par, rrep, mode=kind)
            torch.cuda.synchronize()
            recs = ctx.timing_read()
        finally:
            ctx.timing_enable(False)
        by = {}
        for name, ms, _ in recs:
            by[name] = by.get(name, 0.0) + float(ms)
        return sum(by.values()), by

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

    out = {"shape": {"k": k, "e": e, "len": L, "pitch": enc.pitch, "blocks": B},
           "device": torch.cuda.get_device_name(0), "clean": [], "damaged": []}
    order = ["scrub", "columns", "one_row", "one_row", "columns", "scrub"]
    for rnd in range(a.rounds):
        for pos, kind in enumerate(order):
            ms, by = run(kind)
            out["clean"].append({"round": rnd, "pos": pos, "kind": kind, "ms": ms, "kernels": by})

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

    def stats(v):
        v = np.array(v)
        return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
                "stdev": float(v.std(ddof=1)) if len(v) > 1 else 0.0, "n": int(len(v))}

    summ = {}
    for kind in ("scrub", "columns", "one_row"):
        summ[kind] = stats([r["ms"] for r in out["clean"] if r["kind"] == kind])
    per_round = []
    for rnd in range(a.rounds):
        t = {kd: [r["ms"] for r in out["clean"] if r["round"] == rnd and r["kind"] == kd] for kd in summ}
        sc = sum(t["scrub"]) / 2
        per_round.append({"round": rnd, "scrub_spread": abs(t["scrub"][0] - t["scrub"][1]) / sc,
                          "columns_over_scrub": sum(t["columns"]) / 2 / sc,
                          "one_row_over_scrub": sum(t["one_row"]) / 2 / sc,
                          "one_row_minus_scrub_ms": sum(t["one_row"]) / 2 - sc})
    summ["per_round"] = per_round
    for mode in ("columns", "one_row"):
        summ["damaged_" + mode] = stats([r["ms"] for r in out["damaged"] if r["kind"] == mode])
    gated = [r["kernels"].get("k_rs_bs_repair_gated", 0.0) for r in out["clean"] if r["kind"] == "one_row"]
    summ["one_row_gated_launch_clean"] = stats(gated)
    out["summary"] = summ
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(summ, indent=1))
    ctx.close()


if __name__ == "__main__":
    main()
