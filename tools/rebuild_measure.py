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

With --wide the lists of 9 to 32 rows and the kernel choice are measured
instead (profiles/rebuild_wide/README.md).  Kinds: `threaded_n8`, `_n16`,
`_n32` and `lanes_n8`, `_n16`, `_n32` (rsgpu_set_rebuild_kernel THREADED and
LANES, random full lists, u = n, no check; LANES runs in passes of 8 outputs
above 8), `decode_n8` ... `_n32` (rsgpu_decode_general, the same lists),
`threaded_mixed` and `lanes_mixed` (n drawn from 0 .. 32 per block, u = 32),
`prepare_n8` ... `_n32` and `prepare_mixed` (the wide prepare alone, through
the test hook that stops the call after it) and `copy`.  A list the code does
not determine (BAD_MATRIX) is drawn again before anything is timed.  Besides
the medians the summary holds, for n = 8, 16, 32 and mixed, whether THREADED
was the faster one in every mirrored pair (same round, same half).
"""
import ctypes as C

import numpy as np
import torch

import measure_lib as ml  # puts the engine's directory on the path
import rsgpu  # noqa: E402

UNCHECKED = (1, 2, 4, 8)
CHECKED = (1, 4, 7)


WIDE = (8, 16, 32)


def wide(a):
    k, e, L, B = a.k, a.e, a.len, a.blocks
    ctx, enc = ml.setup(a)
    dev, pitch = enc.src.device, enc.pitch
    rep = ml.reports(enc)
    rng = np.random.default_rng(9)
    hooks = rsgpu.testhooks()
    hooks.rsgpu_internal_set_rebuild_prepare_only.argtypes = [C.c_void_p, C.c_int]

    def draw(n):
        return rsgpu.LOST_NONE if n == 0 else np.sort(rng.choice(k + e, n, replace=False))

    def full(n, u):
        row = np.full(u, rsgpu.LOST_NONE, np.uint8)
        row[:n] = draw(n)
        return row

    nmix = rng.integers(0, min(e, 32) + 1, B)
    lists = {str(n): np.stack([full(n, n) for _ in range(B)]) for n in WIDE}
    lists["mixed"] = np.stack([full(int(n), 32) for n in nmix])
    d_lists = {}

    def call(key, kernel, prepare_only=False):
        u = lists[key].shape[1]
        ctx.set_rebuild_kernel(kernel)
        hooks.rsgpu_internal_set_rebuild_prepare_only(ctx.handle, 1 if prepare_only else 0)
        try:
            ctx.rebuild_blocks(k, e, L, pitch, B, enc.src, enc.par, u, d_lists[key], rep, check=False)
        finally:
            hooks.rsgpu_internal_set_rebuild_prepare_only(ctx.handle, 0)
            ctx.set_rebuild_kernel("auto")

    # lists the code determines: the prepare alone judges them, the rest is drawn again
    redrawn = {}
    for key, v in lists.items():
        for _ in range(20):
            d_lists[key] = torch.from_numpy(v).to(dev)
            call(key, "threaded", prepare_only=True)
            torch.cuda.synchronize()
            bad = np.flatnonzero(rep.cpu().numpy().view(rsgpu.SCRUB_REPORT_DTYPE)["status"] != rsgpu.SCRUB_CLEAN)
            if not len(bad):
                break
            redrawn[key] = redrawn.get(key, 0) + int(len(bad))
            for b in bad:
                n = int((v[b] != rsgpu.LOST_NONE).sum())
                v[b] = full(n, v.shape[1])
        else:
            raise SystemExit(f"lists {key}: still undetermined ones")
    copy_bytes = (k + 4) * L * B // 2
    copy = ml.copy_yardstick(enc, copy_bytes)
    dec_out = torch.empty(B * max(WIDE) * pitch, dtype=torch.uint8, device=dev)
    dec_ws = {n: torch.empty(rsgpu.decode_general_workspace_bytes(k, k + e, n, B), dtype=torch.uint8, device=dev)
              for n in WIDE}
    dec_status = torch.empty(B, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def run(kind):
        if kind == "copy":
            return copy()
        what, key = kind.split("_")
        key = key.lstrip("n")
        if what == "decode":
            n = int(key)
            return ml.timed(ctx, lambda: ctx.decode_general(k, k + e, L, pitch, B, None, enc.src, enc.par,
                                                            d_lists[key], n, dec_out, dec_ws[n], dec_status))
        if what == "prepare":
            return ml.timed(ctx, lambda: call(key, "threaded", prepare_only=True))
        return ml.timed(ctx, lambda: call(key, what))

    keys = [f"n{n}" for n in WIDE] + ["mixed"]
    kinds = ([f"{w}_{key}" for key in keys for w in ("threaded", "lanes")] + [f"decode_n{n}" for n in WIDE] +
             [f"prepare_{key}" for key in keys] + ["copy"])
    kernels_seen = {}
    for kind in kinds:  # untimed and checked
        rep.fill_(0xA5)
        dec_status.fill_(-9)
        _, by = run(kind)
        kernels_seen[kind] = sorted(by)
        if kind.startswith("decode"):
            assert bool((dec_status == 0).all()), kind
        elif kind != "copy":
            assert ml.all_clean(rep), kind
    ctx.scrub_blocks(k, e, L, pitch, B, enc.src, enc.par, rep)
    torch.cuda.synchronize()
    assert ml.all_clean(rep), "the blocks after the rebuilds"

    out = {**ml.header(enc), "kernels": kernels_seen, "redrawn_lists": redrawn,
           "mean_rows_mixed": float(nmix.mean()), "runs": ml.mirrored_rounds(kinds, a.rounds, run)}
    summ = ml.summarise(out["runs"], kinds, kernel_medians=True)
    copy_tb = 2 * copy_bytes / (summ["copy"]["median"] * 1e-3) / 1e12
    summ["copy"]["tb_per_s"] = copy_tb
    half = len(kinds)

    def pairs(x, y):
        """(x ms, y ms) of the runs of a round's same half"""
        at = {(r["round"], r["pos"] >= half, r["kind"]): r["ms"] for r in out["runs"]}
        return [(at[(rnd, h, x)], at[(rnd, h, y)]) for rnd in range(a.rounds) for h in (False, True)]

    for key in keys:
        rows = k + (float(nmix.mean()) if key == "mixed" else int(key[1:]))
        model = rows * L * B / (copy_tb * 1e12) * 1e3
        t, ln = summ[f"threaded_{key}"], summ[f"lanes_{key}"]
        for s in (t, ln):
            s["model_ms"] = model
            s["over_model"] = s["median"] / model
        pr = pairs(f"threaded_{key}", f"lanes_{key}")
        t["over_lanes"] = t["median"] / ln["median"]
        t["faster_than_lanes_in_pairs"] = f"{sum(x < y for x, y in pr)} of {len(pr)}"
        t["prepare_share"] = summ[f"prepare_{key}"]["median"] / t["median"]
        if key != "mixed":
            t["over_decode"] = t["median"] / summ[f"decode_{key}"]["median"]
            ln["over_decode"] = ln["median"] / summ[f"decode_{key}"]["median"]
    ml.finish(a.out, out, summ)
    ctx.close()


def main():
    ap = ml.shape_parser()
    ap.add_argument("--wide", action="store_true", help="lists of up to 32 rows and the kernel choice")
    a = ap.parse_args()
    if a.wide:
        return wide(a)
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
