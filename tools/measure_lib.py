"""What the scrub family's measuring tools share (tools/repair_measure.py,
update_measure.py, degraded_measure.py, rebuild_measure.py, locate_measure.py,
correct_measure.py; a tool, not the
product): the shape arguments, the context and encoder at that shape, the
timing of one call from rsgpu_timing_read, the torch copy that is the
yardstick for "memory-bound", the check that every report is CLEAN, the
mirrored rounds, the statistics per kind and the writer of the result."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "storage-benchmarks_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rsgpu  # noqa: E402


def shape_parser():
    """out [--k 64 --e 32 --len 1000000 --blocks 1024 --rounds 12]; a tool adds its own options."""
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--e", type=int, default=32)
    ap.add_argument("--len", type=int, default=1000000)
    ap.add_argument("--blocks", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=12)
    return ap


def setup(a, coef=None):
    """(context on torch's stream, encoder of the shape with its parity encoded;
    coef: the encoder's parity matrix, None for the built-in code)."""
    ctx = rsgpu.Context(0)
    ctx.set_torch_stream()
    enc = rsgpu.GpuEncoder(a.k, a.len, a.e, blocks=a.blocks, seed=5, ctx=ctx, coef=coef)
    enc.encode_all()
    return ctx, enc


def header(enc):
    """The head of every result: the shape and the device."""
    return {"shape": {"k": enc.k, "e": enc.e, "len": enc.L, "pitch": enc.pitch, "blocks": enc.B},
            "device": torch.cuda.get_device_name(0)}


def reports(enc, dtype=rsgpu.SCRUB_REPORT_DTYPE):
    """Device memory for one report per block."""
    return torch.empty(enc.B * dtype.itemsize, dtype=torch.uint8, device=enc.src.device)


def timed(ctx, fn):
    """One timed run of fn: (ms, {kernel name: ms}), the HIP-event times of
    rsgpu_timing_read summed per kernel name."""
    ctx.timing_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        recs = ctx.timing_read(1 << 16)
    finally:
        ctx.timing_enable(False)
    by = {}
    for name, ms, _ in recs:
        by[name] = by.get(name, 0.0) + float(ms)
    return sum(by.values()), by


def copy_yardstick(enc, nbytes):
    """run() -> (ms, {"copy": ms}): a device-to-device torch copy of nbytes of
    the encoder's sources (nbytes read, nbytes written), HIP events around it."""
    assert nbytes <= enc.src.numel()
    dst = torch.empty(nbytes, dtype=torch.uint8, device=enc.src.device)

    def run():
        a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a0.record()
        dst.copy_(enc.src[:nbytes])
        a1.record()
        torch.cuda.synchronize()
        ms = a0.elapsed_time(a1)
        return ms, {"copy": ms}

    return run


def all_clean(rep):
    """Every scrub report of the device buffer rep is CLEAN with no bad column."""
    r = rep.cpu().numpy().view(rsgpu.SCRUB_REPORT_DTYPE)
    return bool((r["status"] == rsgpu.SCRUB_CLEAN).all() and (r["bad_columns"] == 0).all())


def mirrored_rounds(kinds, rounds, run):
    """`rounds` rounds of the kinds in order and back, every kind twice per
    round: the runs as [{round, pos, kind, ms, kernels}]."""
    order = kinds + kinds[::-1]
    runs = []
    for rnd in range(rounds):
        for pos, kind in enumerate(order):
            ms, by = run(kind)
            runs.append({"round": rnd, "pos": pos, "kind": kind, "ms": ms, "kernels": by})
    return runs


def stats(v):
    v = np.array(v)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
            "stdev": float(v.std(ddof=1)) if len(v) > 1 else 0.0, "n": int(len(v))}


def summarise(runs, kinds, kernel_medians=False):
    """{kind: stats of its runs' ms}, with kernel_medians also kernel_median_ms
    = {kernel name: median ms over the runs, 0 where a run lacks it}."""
    summ = {}
    for kind in kinds:
        mine = [r for r in runs if r["kind"] == kind]
        s = stats([r["ms"] for r in mine])
        if kernel_medians:
            names = sorted({n for r in mine for n in r["kernels"]})
            s["kernel_median_ms"] = {n: float(np.median([r["kernels"].get(n, 0.0) for r in mine])) for n in names}
        summ[kind] = s
    return summ


def dumps(out):
    """The result as JSON with one line per run (per element of every list at
    the top level) and per entry of the summary."""
    parts = []
    for key, v in out.items():
        if isinstance(v, list):
            body = ",\n".join("  " + json.dumps(r) for r in v)
            parts.append(f" {json.dumps(key)}: [\n{body}\n ]")
        elif key == "summary":
            body = ",\n".join(f"  {json.dumps(kind)}: {json.dumps(s)}" for kind, s in v.items())
            parts.append(f' "summary": {{\n{body}\n }}')
        else:
            parts.append(f" {json.dumps(key)}: {json.dumps(v)}")
    return "{\n" + ",\n".join(parts) + "\n}\n"


def finish(path, out, summ):
    """out with its summary into the file, the summary to stdout."""
    out["summary"] = summ
    with open(path, "w") as f:
        f.write(dumps(out))
    print(json.dumps(summ, indent=1))
