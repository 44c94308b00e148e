#!/usr/bin/env python3
"""The degraded scrub's measurement (profiles/degraded/README.md):
rsgpu_scrub_degraded_blocks against the encode, the two scrub kernels and a
plain copy at one shape, in one process on the same buffers.

Kinds: `encode` (rsgpu_encode_blocks: the call's first pass), `degraded_n1`
(one lost row per block, rotating as b mod (k + e)), `degraded_n4` and
`degraded_n8` (random rows of [0, k + e), every block a full list),
`scrub_two_pass` and `scrub_fused` (rsgpu_scrub_blocks, the yardsticks of the
complete-block scrub) and `copy`, a device-to-device copy of (3 + 2 e) len
bytes per block, read plus written, as tools/update_measure.py times it (the
yardstick for "memory-bound").  The survivors are clean and every call runs
with RSGPU_SCRUB_LOCATE, so the cold path never runs; the lost rows hold
their old contents, which the arithmetic does not notice.  After one untimed,
checked run of each kind: `rounds` mirrored rounds, every kind twice per
round.  A run's time is the sum of its kernels' HIP-event times from
rsgpu_timing_read (the copy: HIP events around it).

The byte model: the call costs the encode plus 2 (e - |P|) rows per block
(the stored and the recomputed row of every surviving parity row, P the lost
parity rows) at the copy's rate; `over_model` is measured / modelled.

    python tools/degraded_measure.py out.json [--k 64 --e 32 --len 1000000 --blocks 1024 --rounds 12]
"""
import numpy as np
import torch

import measure_lib as ml  # puts the engine's directory on the path


def main():
    a = ml.shape_parser().parse_args()
    k, e, L, B = a.k, a.e, a.len, a.blocks

    ctx, enc = ml.setup(a)
    dev, pitch = enc.src.device, enc.pitch
    rep = ml.reports(enc)
    rng = np.random.default_rng(9)
    lists = {1: (np.arange(B) % (k + e)).astype(np.uint8).reshape(B, 1)}
    for n in (4, 8):
        lists[n] = np.stack([np.sort(rng.choice(k + e, n, replace=False)) for _ in range(B)]).astype(np.uint8)
    d_lists = {n: torch.from_numpy(v).to(dev) for n, v in lists.items()}
    lost_parity = {n: float((v >= k).sum()) / B for n, v in lists.items()}  # mean |P|
    copy_bytes = (3 + 2 * e) * L * B // 2
    copy = ml.copy_yardstick(enc, copy_bytes)
    scratch_par = torch.empty_like(enc.par)  # the encode kind must not touch the stored parity
    torch.cuda.synchronize()

    def timed(fn):
        return ml.timed(ctx, fn)

    def run(kind):
        """One timed run: (ms, {kernel name: ms})."""
        if kind == "encode":
            return timed(lambda: ctx.encode_blocks(k, e, L, pitch, B, enc.src, scratch_par))
        if kind == "copy":
            return copy()
        if kind.startswith("scrub_"):
            ctx.set_scrub_kernel(kind[len("scrub_"):])
            try:
                return timed(lambda: ctx.scrub_blocks(k, e, L, pitch, B, enc.src, enc.par, rep))
            finally:
                ctx.set_scrub_kernel("auto")
        n = int(kind.split("_n")[1])
        return timed(lambda: ctx.scrub_degraded_blocks(k, e, L, pitch, B, enc.src, enc.par, n, d_lists[n], rep))

    def all_clean():
        return ml.all_clean(rep)

    kinds = ["encode", "degraded_n1", "degraded_n4", "degraded_n8", "scrub_two_pass", "scrub_fused", "copy"]
    kernels_seen = {}
    for kind in kinds:  # untimed and checked
        rep.fill_(0xA5)
        _, by = run(kind)
        kernels_seen[kind] = sorted(by)
        if kind.startswith(("degraded", "scrub")):
            assert all_clean(), kind

    out = {**ml.header(enc), "kernels": kernels_seen, "mean_lost_parity_rows": lost_parity,
           "runs": ml.mirrored_rounds(kinds, a.rounds, run)}
    summ = ml.summarise(out["runs"], kinds, kernel_medians=True)
    copy_tb = 2 * copy_bytes / (summ["copy"]["median"] * 1e-3) / 1e12
    summ["copy"]["tb_per_s"] = copy_tb
    summ["encode"]["tb_per_s"] = (k + e) * L * B / (summ["encode"]["median"] * 1e-3) / 1e12
    for n in (1, 4, 8):
        s = summ[f"degraded_n{n}"]
        rows = 2 * (e - lost_parity[n])
        s["compare_rows_per_block"] = rows
        s["compare_model_ms"] = rows * L * B / (copy_tb * 1e12) * 1e3
        s["model_ms"] = summ["encode"]["median"] + s["compare_model_ms"]
        s["over_model"] = s["median"] / s["model_ms"]
        cmp_ms = sum(v for name, v in s["kernel_median_ms"].items() if name.startswith("k_degraded_compare"))
        s["compare_ms"] = cmp_ms
        s["compare_tb_per_s"] = rows * L * B / (cmp_ms * 1e-3) / 1e12 if cmp_ms else None
        s["compare_over_copy_rate"] = s["compare_tb_per_s"] / copy_tb if cmp_ms else None
        s["over_scrub_two_pass"] = s["median"] / summ["scrub_two_pass"]["median"]
        s["over_scrub_fused"] = s["median"] / summ["scrub_fused"]["median"]
    ml.finish(a.out, out, summ)
    ctx.close()


if __name__ == "__main__":
    main()
