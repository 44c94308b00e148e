#!/usr/bin/env python3
"""The locate's measurement (profiles/locate/README.md): rsgpu_locate_blocks
against the TWO_PASS scrub with RSGPU_SCRUB_LOCATE on the same blocks, clean
and with three kinds of damage, and a plain copy, at one shape, in one process
on the same buffers.

Kinds: `scrub_clean` (rsgpu_scrub_blocks, TWO_PASS, LOCATE) and `locate_clean`
on consistent blocks; `locate_one` (one data row per block, b mod k, bad in 1 %
of the byte columns), `locate_two` (two data rows per block bad in 1 % of the
columns each, different columns), `locate_whole` (two whole data rows per block
bad: every column takes the cooperative path) and `copy`, a device-to-device
copy of (k + 4) len bytes per block, read plus written (the yardstick for
"memory-bound").  Damage is XORed into the rows before a run and XORed out
again after it, outside the timed part, so every kind runs on the same
buffers.  After one untimed, checked run of each kind (the reports and lists
must name exactly the damaged rows): `rounds` mirrored rounds, every kind twice
per round.  A run's time is the sum of its kernels' HIP-event times from
rsgpu_timing_read (the copy: HIP events around it).

Besides the statistics per kind the summary holds locate_clean / scrub_clean
over the mirrored pairs (same round, same half), to be read against the two
kinds' own run-to-run spread.

With --kernel fused (profiles/locate_fused/README.md; two_pass is the default
and measures what is described above) the same process measures both forms:
`fused_scrub_clean` (rsgpu_scrub_blocks, FUSED, LOCATE) and `fused_locate_clean`,
`fused_locate_one`, `fused_locate_two`, `fused_locate_whole` (rsgpu_set_locate_kernel
FUSED), then the four TWO_PASS locate kinds on the same damage, then the copy.
The summary then holds fused_locate_clean / fused_scrub_clean over the mirrored
pairs and every fused locate kind over its TWO_PASS twin.

With --kernel generated (profiles/locate_generated/README.md) the fused form
measured is the generated one, for any matrix (--matrix rs | cauchy: the
built-in gf_gen_rs_matrix code or the Cauchy matrix of the shape):
`generated_scrub_clean` (rsgpu_scrub_blocks, GENERATED, LOCATE) and
`generated_locate_*` (rsgpu_set_locate_kernel FUSED with the scrub kernel
GENERATED), the TWO_PASS twins and the copy, summarised the same way.

    python tools/locate_measure.py out.json [--k 64 --e 32 --len 1000000 --blocks 1024 --rounds 12]
                                            [--kernel {two_pass,fused,generated}] [--matrix {rs,cauchy}]
"""
import numpy as np
import torch

import measure_lib as ml  # puts the engine's directory on the path
import rsgpu  # noqa: E402

DT = rsgpu.SCRUB_REPORT_DTYPE
U = rsgpu.LOCATE_MAX_ROWS


def main():
    ap = ml.shape_parser()
    ap.add_argument("--kernel", choices=["two_pass", "fused", "generated"], default="two_pass")
    ap.add_argument("--matrix", choices=["rs", "cauchy"], default="rs")
    a = ap.parse_args()
    both = a.kernel != "two_pass"
    pre = a.kernel + "_" if both else ""
    # the kernel a fused kind must have run: no silent fall-back to TWO_PASS
    ran = {"fused": ("k_rs_bs_scrub", "k_rs_bs_locate"), "generated": ("k_rs_jit_scrub", "k_rs_jit_locate")}
    k, e, L, B = a.k, a.e, a.len, a.blocks
    coef = None if a.matrix == "rs" else rsgpu.gf_gen_cauchy1_matrix(k + e, k)[k:]
    ctx, enc = ml.setup(a, coef)
    ctx.set_scrub_kernel("two_pass")
    dev, pitch = enc.src.device, enc.pitch
    rep = ml.reports(enc)
    lists = torch.empty(B * U, dtype=torch.uint8, device=dev)
    vs = enc.src.view(B, k, pitch)
    rng = np.random.default_rng(9)
    blk = torch.arange(B, device=dev)
    r1 = torch.arange(B, device=dev) % k
    r2 = (r1 + 1 + torch.from_numpy(rng.integers(0, k - 1, B)).to(dev)) % k  # != r1
    ncols = max(1, L // 100)
    cols = rng.choice(L, min(L, 2 * ncols), replace=False)
    c1 = torch.from_numpy(np.sort(cols[:ncols])).to(dev)
    c2 = torch.from_numpy(np.sort(cols[ncols:])).to(dev) if len(cols) > ncols else c1
    x1 = torch.from_numpy(rng.integers(1, 256, (B, len(c1)), dtype=np.uint8)).to(dev)
    x2 = torch.from_numpy(rng.integers(1, 256, (B, len(c2)), dtype=np.uint8)).to(dev)
    w1 = torch.from_numpy(rng.integers(1, 256, L, dtype=np.uint8)).to(dev)
    w2 = torch.from_numpy(rng.integers(1, 256, L, dtype=np.uint8)).to(dev)

    def sparse(rows, c, x):
        vs[blk[:, None], rows[:, None], c[None, :]] ^= x

    def whole(rows, w):
        vs[blk, rows, :L] ^= w[None, :]

    # the damage of a kind: applying it twice removes it
    damage = {
        "locate_one": lambda: sparse(r1, c1, x1),
        "locate_two": lambda: (sparse(r1, c1, x1), sparse(r2, c2, x2)),
        "locate_whole": lambda: (whole(r1, w1), whole(r2, w2)),
    }
    copy_bytes = (k + 4) * L * B // 2
    copy = ml.copy_yardstick(enc, copy_bytes)
    torch.cuda.synchronize()

    def run(kind):
        """One timed run: (ms, {kernel name: ms})."""
        if kind == "copy":
            return copy()
        form = a.kernel if both and kind.startswith(pre) else "two_pass"
        kind = kind.removeprefix(pre)
        ctx.set_scrub_kernel(form)
        if kind == "scrub_clean":
            return ml.timed(ctx, lambda: ctx.scrub_blocks(k, e, L, pitch, B, enc.src, enc.par, rep, coef=coef))
        ctx.set_locate_kernel("fused" if form == "generated" else form)
        flip = damage.get(kind)
        if flip:
            flip()
            torch.cuda.synchronize()
        try:
            return ml.timed(ctx, lambda: ctx.locate_blocks(k, e, L, pitch, B, enc.src, enc.par, U, lists, rep,
                                                          coef=coef))
        finally:
            if flip:
                flip()
                torch.cuda.synchronize()

    locates = ["locate_clean", "locate_one", "locate_two", "locate_whole"]
    if both:
        kinds = [pre + "scrub_clean", *(pre + n for n in locates), *locates, "copy"]
    else:
        kinds = ["scrub_clean", *locates, "copy"]
    h1, h2 = r1.cpu().numpy(), r2.cpu().numpy()
    lo, hi = np.minimum(h1, h2), np.maximum(h1, h2)
    kernels_seen = {}
    for kind in kinds:  # untimed and checked
        rep.fill_(0xA5)
        lists.fill_(0xA5)
        _, by = run(kind)
        kernels_seen[kind] = sorted(by)
        if kind == "copy":
            continue
        if both and kind.startswith(pre):
            assert ran[a.kernel]["locate" in kind] in by and not any(n.startswith("k_locate_span") for n in by), \
                (kind, sorted(by))
            kind = kind.removeprefix(pre)
        r = rep.cpu().numpy().view(DT)
        got = lists.cpu().numpy().reshape(B, U)
        if kind.endswith("clean"):
            assert ml.all_clean(rep), kind
        elif kind == "locate_one":
            assert (r["status"] == rsgpu.SCRUB_ONE_ROW).all() and (r["row"] == h1).all(), kind
            assert (r["bad_columns"] == len(c1)).all() and (got[:, 0] == h1).all() and (got[:, 1:] == 255).all(), kind
        else:
            assert (r["status"] == rsgpu.SCRUB_ROWS).all() and (r["row"] == lo).all(), kind
            assert (got[:, 0] == lo).all() and (got[:, 1] == hi).all() and (got[:, 2:] == 255).all(), kind
    ctx.set_scrub_kernel("two_pass")
    ctx.scrub_blocks(k, e, L, pitch, B, enc.src, enc.par, rep, coef=coef)
    torch.cuda.synchronize()
    assert ml.all_clean(rep), "the blocks after the damage was taken out again"

    out = {**ml.header(enc), "matrix": a.matrix, "kernels": kernels_seen, "bad_columns_per_row": int(len(c1)),
           "runs": ml.mirrored_rounds(kinds, a.rounds, run)}
    summ = ml.summarise(out["runs"], kinds, kernel_medians=True)
    summ["copy"]["tb_per_s"] = 2 * copy_bytes / (summ["copy"]["median"] * 1e-3) / 1e12
    half = len(kinds)
    at = {(r["round"], r["pos"] >= half, r["kind"]): r["ms"] for r in out["runs"]}
    ratios = [at[(rnd, h, pre + "locate_clean")] / at[(rnd, h, pre + "scrub_clean")] for rnd in range(a.rounds)
              for h in (False, True)]
    summ[pre + "locate_clean"]["over_scrub_in_pairs"] = ml.stats(ratios)
    for kind in kinds[1:-1]:
        summ[kind]["over_scrub"] = summ[kind]["median"] / summ[pre + "scrub_clean"]["median"]
    for kind in locates if both else []:
        summ[pre + kind]["over_two_pass"] = summ[pre + kind]["median"] / summ[kind]["median"]
    ml.finish(a.out, out, summ)
    ctx.set_scrub_kernel("auto")
    ctx.set_locate_kernel("auto")
    ctx.close()


if __name__ == "__main__":
    main()
