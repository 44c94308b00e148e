#!/usr/bin/env python3
"""The rebuild's measurement (profiles/rebuild/README.md): rsgpu_rebuild_blocks
against rsgpu_decode_general (the call it replaces for this step), the
degraded scrub alone and a plain copy at one shape, in one process on the same
buffers.

Kinds: `rebuild_n1` (one lost row per block, rotating as b mod (k + e)),
`rebuild_n2`, `_n4`, `_n8` (random rows of [0, k + e), every block a full
list, u = n), all without RSGPU_REBUILD_CHECK; `checked_n1`, `_n4`, `_n7` (the
same kind of lists with the check, clean survivors); `decode_n1` ... `_n8`
(rsgpu_decode_general with the same lists into a separate buffer);
`degraded_n1`, `_n4`, `_n7` (rsgpu_scrub_degraded_blocks with
RSGPU_SCRUB_LOCATE alone) and `copy`, a device-to-device copy of (k + 4) len
bytes per block, read plus written, as tools/update_measure.py times it (the
yardstick for "memory-bound").  The survivors are clean, so a rebuild writes
into the lost rows what they hold already and every kind sees the same bytes.
After one untimed, checked run of each kind: `rounds` mirrored rounds, every
kind twice per round.  A run's time is the sum of its kernels' HIP-event times
from rsgpu_timing_read (the copy: HIP events around it).

The byte model: a rebuild reads k rows and writes n rows per block at the
copy's rate; the checked call adds the degraded scrub as measured.
`over_model` is measured / modelled, `over_decode` measured / decode_general.

    python tools/rebuild_measure.py out.json [--k 64 --e 32 --len 1000000 --blocks 1024 --rounds 12]
"""
import numpy as np
import torch

import measure_lib as ml  # puts the engine's directory on the path
import rsgpu  # noqa: E402

UNCHECKED = (1, 2, 4, 8)
CHECKED = (1, 4, 7)


def main():
    a = ml.shape_parser().parse_args()
    k, e, L, B = a.k, a.e, a.len, a.blocks

    ctx, enc = ml.setup(a)
    dev, pitch = enc.src.device, enc.pitch
    rep = ml.reports(enc)
    rng = np.random.default_rng(9)
    sizes = sorted(set(UNCHECKED) | set(CHECKED))
    lists = {1: (np.arange(B) % (k + e)).astype(np.uint8).reshape(B, 1)}
    for n in sizes[1:]:
        lists[n] = np.stack([np.sort(rng.choice(k + e, n, replace=False)) for _ in range(B)]).astype(np.uint8)
    d_lists = {n: torch.from_numpy(v).to(dev) for n, v in lists.items()}
    lost_parity = {n: float((v >= k).sum()) / B for n, v in lists.items()}  # mean |P|
    copy_bytes = (k + 4) * L * B // 2
    copy = ml.copy_yardstick(enc, copy_bytes)
    # rsgpu_decode_general's output rows, workspace and statuses
    dec_out = torch.empty(B * max(sizes) * pitch, dtype=torch.uint8, device=dev)
    dec_ws = {n: torch.empty(rsgpu.decode_general_workspace_bytes(k, k + e, n, B), dtype=torch.uint8, device=dev)
              for n in UNCHECKED}
    dec_status = torch.empty(B, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def timed(fn):
        return ml.timed(ctx, fn)

    def run(kind):
        """One timed run: (ms, {kernel name: ms})."""
        if kind == "copy":
            return copy()
        what, n = kind.split("_n")
        n = int(n)
        if what == "decode":
            return timed(lambda: ctx.decode_general(k, k + e, L, pitch, B, None, enc.src, enc.par, d_lists[n], n,
                                                    dec_out, dec_ws[n], dec_status))
        if what == "degraded":
            return timed(lambda: ctx.scrub_degraded_blocks(k, e, L, pitch, B, enc.src, enc.par, n, d_lists[n],
                                                           rep))
        return timed(lambda: ctx.rebuild_blocks(k, e, L, pitch, B, enc.src, enc.par, n, d_lists[n], rep,
                                                check=what == "checked"))

    def all_clean():
        return ml.all_clean(rep)

    kinds = ([f"rebuild_n{n}" for n in UNCHECKED] + [f"checked_n{n}" for n in CHECKED] +
             [f"decode_n{n}" for n in UNCHECKED] + [f"degraded_n{n}" for n in CHECKED] + ["copy"])
    kernels_seen = {}
    for kind in kinds:  # untimed and checked
        rep.fill_(0xA5)
        dec_status.fill_(-9)
        _, by = run(kind)
        kernels_seen[kind] = sorted(by)
        if kind.startswith("decode"):
            assert bool((dec_status == 0).all()), kind
        elif kind != "copy":
            assert all_clean(), kind
    # the rebuilds wrote into the blocks: they are still the encode
    ctx.scrub_blocks(k, e, L, pitch, B, enc.src, enc.par, rep)
    torch.cuda.synchronize()
    assert all_clean(), "the blocks after the rebuilds"

    out = {**ml.header(enc), "kernels": kernels_seen, "mean_lost_parity_rows": lost_parity,
           "runs": ml.mirrored_rounds(kinds, a.rounds, run)}
    summ = ml.summarise(out["runs"], kinds, kernel_medians=True)
    copy_tb = 2 * copy_bytes / (summ["copy"]["median"] * 1e-3) / 1e12
    summ["copy"]["tb_per_s"] = copy_tb
    for n in UNCHECKED:
        s = summ[f"rebuild_n{n}"]
        s["rows_per_block"] = k + n
        s["model_ms"] = (k + n) * L * B / (copy_tb * 1e12) * 1e3
        s["over_model"] = s["median"] / s["model_ms"]
        hot = sum(v for name, v in s["kernel_median_ms"].items() if name.startswith("k_rebuild_blocks"))
        s["kernel_ms"] = hot
        s["kernel_tb_per_s"] = (k + n) * L * B / (hot * 1e-3) / 1e12
        s["kernel_over_copy_rate"] = s["kernel_tb_per_s"] / copy_tb
        s["over_decode"] = s["median"] / summ[f"decode_n{n}"]["median"]
    for n in CHECKED:
        s = summ[f"checked_n{n}"]
        s["model_ms"] = summ[f"degraded_n{n}"]["median"] + (k + n) * L * B / (copy_tb * 1e12) * 1e3
        s["over_model"] = s["median"] / s["model_ms"]
        s["over_degraded"] = s["median"] / summ[f"degraded_n{n}"]["median"]
    ml.finish(a.out, out, summ)
    ctx.close()


if __name__ == "__main__":
    main()
