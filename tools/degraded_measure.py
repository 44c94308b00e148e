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

--kernel two_pass | fused runs the degraded kinds above under that choice of
rsgpu_set_degraded_kernel.  --kernel both is the measurement of the fused form
(profiles/degraded_fused/README.md) instead: every case under FUSED and under
TWO_PASS in mirrored pairs in one process -- clean blocks with all-NONE lists
(beside the FUSED rsgpu_scrub_blocks), one lost data row, one lost parity
row, 4 lost rows, 8 lost data rows and mixed lists of 0 to 8 rows; one
surviving row bad in 1 % of the columns with one lost data row; the checked
rebuild at n = 1, 4, 7 with clean survivors -- after one untimed run of each
whose reports must be equal byte for byte under both choices.  Per case:
the medians, and min / median / max of the ratio FUSED / TWO_PASS over the
pairs of a round's two halves.

--generated --matrix rs | cauchy is the same measurement of the generated form
(profiles/degraded_generated/README.md): the matrix is passed as `coef`
(gf_gen_rs_matrix, so that a compiled code does not take the compiled form, or
gf_gen_cauchy1_matrix), the first side runs under FUSED with the scrub kernel
GENERATED (k_rs_jit_degraded), and the yardstick beside the all-NONE case is
the GENERATED rsgpu_scrub_blocks with LOCATE.  The summary also holds the
ratio all-NONE / yardstick over the mirrored pairs beside the yardstick's own
first-half / second-half spread, measured in the same run.
"""
import numpy as np
import torch

import measure_lib as ml  # puts the engine's directory on the path


def both(a, ctx, enc, coef=None):
    """--kernel both: FUSED against TWO_PASS, case by case; with `coef`
    (--generated): FUSED under the scrub kernel GENERATED against TWO_PASS."""
    k, e, L, B = a.k, a.e, a.len, a.blocks
    gen = coef is not None
    yard = "scrub_generated" if gen else "scrub_fused"  # the scrub of the complete blocks
    form = "k_rs_jit_degraded" if gen else "k_rs_bs_degraded"
    dev, pitch = enc.src.device, enc.pitch
    rep = ml.reports(enc)
    rng = np.random.default_rng(9)
    none = np.full((B, 1), 255, np.uint8)

    def pad(rows, u):
        return np.concatenate([np.sort(rows), np.full(u - len(rows), 255)]).astype(np.uint8)

    lists = {
        "none": none,
        "data1": (np.arange(B) % k).astype(np.uint8).reshape(B, 1),
        "parity1": (k + np.arange(B) % e).astype(np.uint8).reshape(B, 1),
        # (a small code: no more rows than it has parity rows, or data rows)
        "rows4": np.stack([pad(rng.choice(k + e, min(4, e), replace=False), 4) for _ in range(B)]),
        "data8": np.stack([pad(rng.choice(k, min(8, e, k), replace=False), 8) for _ in range(B)]),
        "mixed": np.stack([pad(rng.choice(k + e, b % (min(8, e) + 1), replace=False), 8) for b in range(B)]),
    }
    for n in (1, 4, 7):
        lists[f"rebuild{n}"] = np.stack([pad(rng.choice(k + e, min(n, max(1, e - 1)), replace=False), n)
                                         for _ in range(B)])
    lists["bad1pct"] = lists["data1"]
    d_lists = {n: torch.from_numpy(v).to(dev) for n, v in lists.items()}
    cases = list(lists)
    # bad1pct: row (lost + 1) mod k of every block, bad in every 100th column; applied around its runs
    cols = torch.arange(0, L, 100, device=dev)
    bad_rows = torch.from_numpy((lists["data1"][:, 0].astype(np.int64) + 1) % k).to(dev)
    src = enc.src.view(B, k, pitch)

    def flip():
        src[torch.arange(B, device=dev)[:, None], bad_rows[:, None], cols[None, :]] ^= 0x5A

    def run(kind):
        case, kernel = kind.rsplit("/", 1)
        if case == yard:
            ctx.set_scrub_kernel("generated" if gen else "fused")
            try:
                return ml.timed(ctx, lambda: ctx.scrub_blocks(k, e, L, pitch, B, enc.src, enc.par, rep, coef=coef))
            finally:
                ctx.set_scrub_kernel("auto")
        ctx.set_degraded_kernel(kernel)
        if gen and kernel == "fused":
            ctx.set_scrub_kernel("generated")
        lst = d_lists[case]
        u = lst.shape[1]
        if case == "bad1pct":
            flip()
        try:
            if case.startswith("rebuild"):
                return ml.timed(ctx, lambda: ctx.rebuild_blocks(k, e, L, pitch, B, enc.src, enc.par, u, lst, rep,
                                                                coef=coef, check=True))
            return ml.timed(ctx, lambda: ctx.scrub_degraded_blocks(k, e, L, pitch, B, enc.src, enc.par, u, lst, rep,
                                                                   coef=coef))
        finally:
            ctx.set_degraded_kernel("auto")
            ctx.set_scrub_kernel("auto")
            if case == "bad1pct":
                flip()

    kinds = [f"{c}/{kern}" for c in cases for kern in ("fused", "two_pass")] + [f"{yard}/-"]
    kernels_seen, statuses = {}, {}
    for c in cases:  # untimed and checked: the same reports under both choices
        got = {}
        for kern in ("fused", "two_pass"):
            rep.fill_(0xA5)
            _, by = run(f"{c}/{kern}")
            kernels_seen[f"{c}/{kern}"] = sorted(by)
            got[kern] = rep.cpu().numpy().tobytes()
        assert got["fused"] == got["two_pass"], c
        assert form in kernels_seen[f"{c}/fused"], kernels_seen
        r = np.frombuffer(got["fused"], ml.rsgpu.SCRUB_REPORT_DTYPE)
        statuses[c] = {int(v): int((r["status"] == v).sum()) for v in np.unique(r["status"])}
        if c != "bad1pct":
            assert (r["bad_columns"] == 0).all(), c
    run(f"{yard}/-")
    out = {**ml.header(enc), "kernels": kernels_seen, "statuses": statuses,
           "runs": ml.mirrored_rounds(kinds, a.rounds, run)}
    summ = ml.summarise(out["runs"], kinds, kernel_medians=True)
    for c in cases:
        ratios = []
        for rnd in range(a.rounds):
            mine = [r for r in out["runs"] if r["round"] == rnd]
            for half in (mine[:len(kinds)], mine[len(kinds):]):
                ms = {r["kind"]: r["ms"] for r in half}
                ratios.append(ms[f"{c}/fused"] / ms[f"{c}/two_pass"])
        summ[f"{c}/fused"]["pair_ratio_to_two_pass"] = {"min": float(min(ratios)), "median": float(np.median(ratios)),
                                                        "max": float(max(ratios))}
    # all-NONE against the scrub of the complete blocks, and the yardstick's own spread
    ratios, own = [], []
    for rnd in range(a.rounds):
        mine = [r for r in out["runs"] if r["round"] == rnd]
        first, second = ({r["kind"]: r["ms"] for r in h} for h in (mine[:len(kinds)], mine[len(kinds):]))
        ratios += [first["none/fused"] / first[f"{yard}/-"], second["none/fused"] / second[f"{yard}/-"]]
        own.append(first[f"{yard}/-"] / second[f"{yard}/-"])
    summ["none/fused"]["pair_ratio_to_scrub"] = {**ml.stats(ratios), "mean": float(np.mean(ratios))}
    summ[f"{yard}/-"]["first_over_second_half"] = {**ml.stats(own), "mean": float(np.mean(own))}
    ml.finish(a.out, out, summ)


def main():
    ap = ml.shape_parser()
    ap.add_argument("--kernel", choices=("auto", "two_pass", "fused", "both"), default="auto")
    ap.add_argument("--generated", action="store_true", help="the generated form against TWO_PASS, as --kernel both")
    ap.add_argument("--matrix", choices=["rs", "cauchy"], default="rs", help="with --generated: the matrix, as coef")
    a = ap.parse_args()
    k, e, L, B = a.k, a.e, a.len, a.blocks

    coef = None
    if a.generated:
        gen = ml.rsgpu.gf_gen_rs_matrix if a.matrix == "rs" else ml.rsgpu.gf_gen_cauchy1_matrix
        coef = gen(k + e, k)[k:]
    ctx, enc = ml.setup(a, coef)
    if a.kernel == "both" or a.generated:
        both(a, ctx, enc, coef)
        ctx.close()
        return
    ctx.set_degraded_kernel(a.kernel)
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
