#!/usr/bin/env python3
"""The generated scrub's measurement (profiles/scrub_generated/README.md): per
code, in one process on the same buffers, the scrub under `generated` against
its yardsticks -- the TWO_PASS scrub, the GENERATED encode of the same rows
into a spare buffer and, where the code is compiled, the FUSED scrub.

Per code: one untimed, checked run of each kind (every report CLEAN, the spare
parity equal to the stored one), then `rounds` mirrored rounds of the kinds in
order and back on clean data, with RSGPU_SCRUB_LOCATE.  A run's time is the sum
of its kernels' HIP-event times from rsgpu_timing_read; the kernels' names and
their median times are kept.  `--bytes` of rows per batch (k + e rows of `len`
per block) fix the block count of every code.

    python tools/scrub_measure.py out.json [--len 1000000 --bytes 1500000000 --rounds 12
                                            --codes 10,4,rs 10,4,cauchy 20,7,rs 64,32,rs]
"""
import argparse

import torch

import measure_lib as ml  # puts the engine's directory on the path
import rsgpu  # noqa: E402

COMPILED = {(16, 4), (16, 8), (64, 32), (64, 16), (100, 20), (5, 4), (20, 7)}


def measure(ctx, k, e, kind, L, nbytes, rounds):
    B = max(1, round(nbytes / ((k + e) * L)))
    coef = None if kind == "rs" else rsgpu.gf_gen_cauchy1_matrix(k + e, k)[k:]
    enc = rsgpu.GpuEncoder(k, L, e, blocks=B, seed=5, ctx=ctx)
    ctx.encode_blocks(k, e, L, enc.pitch, B, enc.src, enc.par, coef=coef)
    spare = torch.zeros_like(enc.par)
    rep = ml.reports(enc)
    kinds = ["generated", "two_pass", "encode_generated"] + (["fused"] if kind == "rs" and (k, e) in COMPILED else [])

    def run(what):
        if what == "encode_generated":
            ctx.set_encode_kernel("generated")
            try:
                return ml.timed(ctx, lambda: ctx.encode_blocks(k, e, L, enc.pitch, B, enc.src, spare, coef=coef))
            finally:
                ctx.set_encode_kernel("auto")
        ctx.set_scrub_kernel(what)
        try:
            rep.fill_(0xA5)
            return ml.timed(ctx, lambda: ctx.scrub_blocks(k, e, L, enc.pitch, B, enc.src, enc.par, rep, coef=coef))
        finally:
            ctx.set_scrub_kernel("auto")

    expect = {"generated": "k_rs_jit_scrub", "two_pass": "k_scrub_compare", "encode_generated": "k_rs_jit(encode)",
              "fused": "k_rs_bs_scrub"}
    for what in kinds:  # untimed and checked
        _, by = run(what)
        assert expect[what] in by, (what, by)
        if what == "encode_generated":
            rows = lambda t: t.view(B, e, enc.pitch)[:, :, :L]  # noqa: E731
            assert torch.equal(rows(spare), rows(enc.par))
        else:
            assert ml.all_clean(rep), what
    runs = ml.mirrored_rounds(kinds, rounds, run)
    summ = ml.summarise(runs, kinds, kernel_medians=True)
    g = summ["generated"]["median"]
    ratios = {f"generated/{o}": g / summ[o]["median"] for o in kinds[1:]}
    return {"code": {"k": k, "e": e, "matrix": kind, "len": L, "pitch": enc.pitch, "blocks": B,
                     "row_bytes": B * (k + e) * L},
            "summary": summ, "ratios": ratios, "runs": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--len", type=int, default=1000000)
    ap.add_argument("--bytes", type=float, default=1.5e9)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--codes", nargs="*", default=["10,4,rs", "10,4,cauchy", "20,7,rs", "64,32,rs"])
    a = ap.parse_args()
    ctx = rsgpu.Context(0)
    ctx.set_torch_stream()
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "codes": []}
    table = {}
    for code in a.codes:
        k, e, kind = code.split(",")
        r = measure(ctx, int(k), int(e), kind, a.len, a.bytes, a.rounds)
        out["codes"].append(r)
        table[code] = {"blocks": r["code"]["blocks"],
                       **{w: [round(s[x], 3) for x in ("median", "min", "max")] for w, s in r["summary"].items()},
                       **{n: round(v, 3) for n, v in r["ratios"].items()}}
    ml.finish(a.out, out, table)
    ctx.close()


if __name__ == "__main__":
    main()
