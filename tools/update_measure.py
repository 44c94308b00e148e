#!/usr/bin/env python3
"""The partial-stripe update's measurement (profiles/update/README.md):
rsgpu_update_blocks against re-encoding and against a plain copy at one shape,
in one process on the same buffers.

Kinds: `encode` (rsgpu_encode_blocks, the yardstick for "cheaper than
re-encoding"), `update_uN` for N listed rows per block (random rows, every
block a full list), `update_u1_delta` (RSGPU_UPDATE_DELTA), and `copy`, a
device-to-device copy that moves as many bytes as the u = 1 update does
((3 + 2 e) len per block, read plus written; the yardstick for "memory-bound").
After one untimed, checked run of each kind: `rounds` mirrored rounds, every
kind twice per round.  A run's time is the sum of its kernels' HIP-event times
from rsgpu_timing_read (the copy: HIP events around it).  Every update is
checked by the scrub that follows the rounds: all blocks CLEAN (the delta kind
runs an even number of times on the same rows, so it cancels).  Once, outside
the rounds: the per-block loop over rsgpu_ec_encode_data_update for u = 1.

    python tools/update_measure.py out.json [--k 64 --e 32 --len 1000000 --blocks 1024 --rounds 12]
"""
import time

import numpy as np
import torch

import measure_lib as ml  # puts the engine's directory on the path
import rsgpu  # noqa: E402

GROUP = 8  # rows of a list one walk over the parity serves (rs_update.hip)


def main():
    ap = ml.shape_parser()
    ap.add_argument("--counts", default="1,4,8,9,16,32")
    a = ap.parse_args()
    k, e, L, B = a.k, a.e, a.len, a.blocks
    counts = [int(x) for x in a.counts.split(",")]
    umax = max(counts)

    ctx, enc = ml.setup(a)
    dev, pitch = enc.src.device, enc.pitch
    upd = torch.empty(B * umax * pitch, dtype=torch.uint8, device=dev)
    ctx.fill_synthetic(upd, B * umax, L, pitch, 77, 0)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    srep = ml.reports(enc)
    rng = np.random.default_rng(9)
    lists = {u: np.stack([np.sort(rng.choice(k, u, replace=False)) for _ in range(B)]).astype(np.uint8)
             for u in counts}
    d_lists = {u: torch.from_numpy(v).to(dev) for u, v in lists.items()}
    # the copy: as many bytes as the u = 1 update moves, half read, half written
    copy_bytes = (3 + 2 * e) * L * B // 2
    copy = ml.copy_yardstick(enc, copy_bytes)
    torch.cuda.synchronize()

    def timed(fn):
        return ml.timed(ctx, fn)

    def run(kind):
        """One timed run: (ms, {kernel name: ms})."""
        if kind == "encode":
            return timed(lambda: ctx.encode_blocks(k, e, L, pitch, B, enc.src, enc.par))
        if kind == "copy":
            return copy()
        delta = kind.endswith("_delta")
        u = int(kind.split("_")[1][1:])
        return timed(lambda: ctx.update_blocks(k, e, L, pitch, B, u, d_lists[u], upd, None if delta else enc.src,
                                               enc.par, status, delta=delta))

    def all_clean():
        ctx.scrub_blocks(k, e, L, pitch, B, enc.src, enc.par, srep)
        torch.cuda.synchronize()
        return ml.all_clean(srep)

    kinds = ["encode"] + [f"update_u{u}" for u in counts] + ["update_u1_delta", "copy"]
    # untimed and checked, one run of each kind
    assert all_clean()
    for kind in kinds:
        run(kind)
        if kind.startswith("update"):
            assert (status.cpu().numpy() == 0).all(), kind
        if kind.endswith("_delta"):
            assert not all_clean()  # the parity moved, the sources did not
            run(kind)               # the same deltas again cancel
        assert all_clean(), kind

    out = {**ml.header(enc), "runs": ml.mirrored_rounds(kinds, a.rounds, run)}
    assert all_clean(), "after the rounds"

    # once: the pointer form, one call per block, u = 1 (the update row taken
    # as the delta; a second, untimed loop cancels it)
    g = rsgpu.ec_init_tables(k, e, rsgpu.gf_gen_rs_matrix(k + e, k)[k:])
    par = enc.par.data_ptr()

    def loop():
        for b in range(B):
            ctx.ec_encode_data_update(L, k, e, int(lists[1][b, 0]), g, upd.data_ptr() + b * pitch,
                                      [par + (b * e + p) * pitch for p in range(e)])

    a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a0.record()
    loop()
    a1.record()
    t_enq = time.perf_counter() - t0
    torch.cuda.synchronize()
    t_wall = time.perf_counter() - t0
    out["pointer_form_u1"] = {"calls": B, "device_ms": a0.elapsed_time(a1), "enqueue_ms": t_enq * 1e3,
                              "wall_ms": t_wall * 1e3}
    loop()
    assert all_clean(), "after the pointer form"

    def rows_moved(kind):
        """Rows of len bytes per block, read plus written (the byte model)."""
        if kind == "encode":
            return k + e
        if kind == "copy":
            return 2 * copy_bytes / (L * B)
        u = int(kind.split("_")[1][1:])
        passes = (u + GROUP - 1) // GROUP
        return (u if kind.endswith("_delta") else 3 * u) + 2 * e * passes

    summ = ml.summarise(out["runs"], kinds)
    for kind in kinds:
        s = summ[kind]
        s["rows_moved_per_block"] = rows_moved(kind)
        s["bytes"] = rows_moved(kind) * L * B
        s["tb_per_s"] = s["bytes"] / (s["median"] * 1e-3) / 1e12
    copy_rate = summ["copy"]["tb_per_s"]
    for kind in kinds:
        summ[kind]["rate_over_copy"] = summ[kind]["tb_per_s"] / copy_rate
    # the alternative to an update of u rows: copy the new rows in (u rows read,
    # u written, at the copy's measured rate), then re-encode
    ms_per_row = summ["copy"]["median"] / summ["copy"]["rows_moved_per_block"]
    for u in counts:
        alt = summ["encode"]["median"] + 2 * u * ms_per_row
        summ[f"update_u{u}"]["copy_in_then_encode_ms"] = alt
        summ[f"update_u{u}"]["update_over_alternative"] = summ[f"update_u{u}"]["median"] / alt
    per_round = []
    for rnd in range(a.rounds):
        t = {kd: [r["ms"] for r in out["runs"] if r["round"] == rnd and r["kind"] == kd] for kd in kinds}
        per_round.append({"round": rnd, "encode_ms": t["encode"], "update_u1_ms": t["update_u1"],
                          "u1_faster_than_encode": max(t["update_u1"]) < min(t["encode"]),
                          "u1_over_encode": sum(t["update_u1"]) / sum(t["encode"]),
                          "u1_over_copy": sum(t["update_u1"]) / sum(t["copy"])})
    summ["per_round"] = per_round
    summ["u1_faster_than_encode_in_every_round"] = all(r["u1_faster_than_encode"] for r in per_round)
    ml.finish(a.out, out, summ)
    ctx.close()


if __name__ == "__main__":
    main()
