#!/usr/bin/env python3
"""The measurements of rsgpu_ec_encode_data_batch (profiles/ec_batch/README.md),
each in one process, in mirrored rounds (tools/measure_lib.py), after one
untimed run of every kind whose output is checked against the yardstick's.

    python tools/ec_batch_measure.py out.json --what a|b|c [--rounds 12] [--blocks N]

a  The same bytes through the same kernel body: (64, 32) gf_gen_rs_matrix
   tables, len 1 000 000, 1024 blocks, the tables pointing into one contiguous
   arena, aligned32.  Yardstick: rsgpu_encode_blocks with a `coef` of the same
   matrix under set_encode_kernel("generated"), measured twice per half round
   (`blocks_a`, `blocks_b`), so that the spread of the yardstick against itself
   stands beside the ratio batch / yardstick.  A run's time is the sum of its
   kernels' HIP-event times from rsgpu_timing_read.
b  What the call is for: 4096 stripes of (10, 4) x 65536 bytes, rows scattered
   over one arena in random order.  Yardstick: 4096 rsgpu_ec_encode_data calls.
   A run's time is the time between two HIP events around the whole run on the
   context's stream (timing records off: the yardstick is bound by its
   launches, which its kernels' own times do not show), and the host's wall
   clock beside it.
c  Skew: one stripe of 1 MiB and 4095 of 4 KiB under max_len 1 MiB, against
   the same total bytes at one length (4352), (10, 4), with and without
   aligned32.  Times as in (b); the kernels' own times from one more run with
   the timing records on.  The difference is what the workgroups that find
   nothing to do cost.
"""
import ctypes
import time

import numpy as np
import torch

import measure_lib as ml  # puts the engine's directory on the path

rsgpu = ml.rsgpu


def bracket(fn):
    """(ms between two HIP events around fn on the current stream, host ms)."""
    a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a0.record()
    fn()
    a1.record()
    torch.cuda.synchronize()
    return a0.elapsed_time(a1), (time.perf_counter() - t0) * 1e3


def pair_ratios(runs, kinds, num, den, rounds):
    """num / den over the two halves of every round."""
    out = []
    for rnd in range(rounds):
        mine = [r for r in runs if r["round"] == rnd]
        for half in (mine[:len(kinds)], mine[len(kinds):]):
            ms = {r["kind"]: r["ms"] for r in half}
            out.append(ms[num] / ms[den])
    return {"min": float(min(out)), "median": float(np.median(out)), "max": float(max(out))}


def tables(dev, src_ptrs, out_ptrs, lens):
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)  # noqa: E731
    return t(src_ptrs, np.int64), t(out_ptrs, np.int64), t(lens, np.int32)


def what_a(a):
    k, e, L, B = 64, 32, 1000000, a.blocks or 1024
    ctx = rsgpu.Context(0)
    ctx.set_torch_stream()
    c = rsgpu.gf_gen_rs_matrix(k + e, k)[k:].copy()
    g = rsgpu.ec_init_tables(k, e, c)
    enc = rsgpu.GpuEncoder(k, L, e, blocks=B, seed=5, ctx=ctx, coef=c)
    dev, pitch = enc.src.device, enc.pitch
    sp = enc.src.data_ptr() + (np.arange(B * k, dtype=np.int64) * pitch).reshape(B, k)
    op = enc.par.data_ptr() + (np.arange(B * e, dtype=np.int64) * pitch).reshape(B, e)
    d_data, d_coding, d_len = tables(dev, sp, op, np.full(B, L))
    status = torch.empty(B, dtype=torch.int32, device=dev)
    ctx.set_encode_kernel("generated")

    def run(kind):
        if kind == "batch":
            return ml.timed(ctx, lambda: ctx.ec_encode_data_batch(k, e, g, B, d_data, d_coding, d_len, L, status,
                                                                  aligned32=True))
        return ml.timed(ctx, lambda: enc.encode_all())

    def digest():
        par = enc.par[: B * e * pitch].view(B, e, pitch)[:, :, :L]
        return int(enc.par[: B * e * pitch // 8 * 8].view(torch.int64).sum().item()), par[:: max(1, B // 8)].clone()

    kinds = ["blocks_a", "batch", "blocks_b"]
    enc.par.fill_(0x3C)
    _, seen_blocks = run("blocks_a")
    want = digest()
    enc.par.fill_(0x3C)
    _, seen_batch = run("batch")
    got = digest()
    assert got[0] == want[0] and torch.equal(got[1], want[1]), "the batch call's parity differs"
    assert not status.any()
    del want, got
    out = {"what": "a", **ml.header(enc), "kernels": {"blocks": sorted(seen_blocks), "batch": sorted(seen_batch)},
           "runs": ml.mirrored_rounds(kinds, a.rounds, run)}
    summ = ml.summarise(out["runs"], kinds, kernel_medians=True)
    summ["batch"]["pair_ratio_to_blocks_a"] = pair_ratios(out["runs"], kinds, "batch", "blocks_a", a.rounds)
    summ["blocks_b"]["pair_ratio_to_blocks_a"] = pair_ratios(out["runs"], kinds, "blocks_b", "blocks_a", a.rounds)
    ml.finish(a.out, out, summ)
    ctx.close()


def scattered(ctx, k, e, lens, slot, seed=3):
    """Blocks of (k, e) rows, block b lens[b] bytes long, every row in a slot of
    `slot` bytes of one arena, the slots in random order.  Returns (arena,
    source pointers [B, k], output pointers [B, e])."""
    B = len(lens)
    dev = torch.device("cuda", 0)
    arena = torch.empty(B * (k + e) * slot, dtype=torch.uint8, device=dev)
    ctx.fill_synthetic(arena, B * (k + e), slot, slot, 7, 0)
    order = np.random.default_rng(seed).permutation(B * (k + e)).astype(np.int64).reshape(B, k + e)
    ptrs = arena.data_ptr() + order * slot
    return arena, np.ascontiguousarray(ptrs[:, :k]), np.ascontiguousarray(ptrs[:, k:])


def outputs(arena, op, lens, base, pick):
    """The output rows of the blocks `pick`, end to end (a device tensor)."""
    return torch.cat([arena[int(p) - base: int(p) - base + int(lens[b])] for b in pick for p in op[b]])


def what_b(a):
    k, e, L, B = 10, 4, 65536, a.blocks or 4096
    ctx = rsgpu.Context(0)
    ctx.set_torch_stream()
    c = rsgpu.gf_gen_rs_matrix(k + e, k)[k:].copy()
    g = rsgpu.ec_init_tables(k, e, c)
    lens = np.full(B, L)
    arena, sp, op = scattered(ctx, k, e, lens, L)
    d_data, d_coding, d_len = tables(arena.device, sp, op, lens)
    status = torch.empty(B, dtype=torch.int32, device=arena.device)
    # the yardstick's calls straight through ctypes on arrays made once, so
    # that as little as possible of the wrapper's own time is in its launches
    vp, fn, gp = ctypes.c_void_p, rsgpu.lib().rsgpu_ec_encode_data, g.ctypes.data
    rows = [((vp * k)(*[int(p) for p in sp[b]]), (vp * e)(*[int(p) for p in op[b]])) for b in range(B)]
    pick = range(0, B, max(1, B // 64))

    def loop():
        for s, o in rows:
            if fn(ctx.handle, L, k, e, gp, s, o):
                raise RuntimeError("rsgpu_ec_encode_data failed")

    calls = {"loop": loop,
             "batch": lambda: ctx.ec_encode_data_batch(k, e, g, B, d_data, d_coding, d_len, L, status),
             "batch_aligned32": lambda: ctx.ec_encode_data_batch(k, e, g, B, d_data, d_coding, d_len, L, status,
                                                                 aligned32=True)}
    kinds = list(calls)
    seen, ref, wall = {}, None, {}
    for kind in kinds:  # untimed and checked: the same output rows
        for b in pick:
            for p in op[b]:
                arena[int(p) - arena.data_ptr():][:L].fill_(0x3C)
        _, by = ml.timed(ctx, calls[kind])
        seen[kind] = {n: round(v, 4) for n, v in by.items()}
        got = outputs(arena, op, lens, arena.data_ptr(), pick)
        ref = got if ref is None else ref
        assert torch.equal(got, ref), kind

    def run(kind):
        ms, host = bracket(calls[kind])
        wall.setdefault(kind, []).append(host)
        return ms, {}

    out = {"what": "b", "shape": {"k": k, "rows": e, "len": L, "blocks": B}, "device": torch.cuda.get_device_name(0),
           "kernel_ms_of_one_run": seen, "runs": ml.mirrored_rounds(kinds, a.rounds, run)}
    summ = ml.summarise(out["runs"], kinds)
    for kind in kinds:
        summ[kind]["host_wall_ms_median"] = float(np.median(wall[kind]))
        if kind != "loop":
            summ[kind]["pair_ratio_to_loop"] = pair_ratios(out["runs"], kinds, kind, "loop", a.rounds)
    ml.finish(a.out, out, summ)
    ctx.close()


def what_c(a):
    k, e, B = 10, 4, a.blocks or 4096
    big, small = 1 << 20, 4096
    ctx = rsgpu.Context(0)
    ctx.set_torch_stream()
    c = rsgpu.gf_gen_rs_matrix(k + e, k)[k:].copy()
    g = rsgpu.ec_init_tables(k, e, c)
    skew = np.full(B, small)
    skew[B // 2] = big
    uni_len = (int(skew.sum()) // B + 31) // 32 * 32
    uni = np.full(B, uni_len)
    sets = {}
    for name, lens in (("skew", skew), ("uniform", uni)):
        if name == "skew":  # the long stripe in an arena of its own
            arena, sp, op = scattered(ctx, k, e, lens, small)
            long_rows = torch.empty((k + e) * big, dtype=torch.uint8, device=arena.device)
            ctx.fill_synthetic(long_rows, k + e, big, big, 9, 0)
            p = long_rows.data_ptr() + np.arange(k + e, dtype=np.int64) * big
            sp[B // 2], op[B // 2] = p[:k], p[k:]
            keep = (arena, long_rows)
        else:
            arena, sp, op = scattered(ctx, k, e, lens, uni_len)
            keep = (arena,)
        d_data, d_coding, d_len = tables(arena.device, sp, op, lens)
        sets[name] = (keep, d_data, d_coding, d_len, int(lens.max()), sp, op, lens)
    status = torch.empty(B, dtype=torch.int32, device=torch.device("cuda", 0))

    def call(kind):
        name, mode = kind.split("/")
        _, d_data, d_coding, d_len, max_len = sets[name][:5]
        return lambda: ctx.ec_encode_data_batch(k, e, g, B, d_data, d_coding, d_len, max_len, status,
                                                aligned32=mode == "aligned32")

    kinds = [f"{n}/{m}" for m in ("aligned32", "default") for n in ("skew", "uniform")]
    seen, wall = {}, {}
    for kind in kinds:  # untimed; a block's rows against rsgpu_ec_encode_data on a copy
        _, by = ml.timed(ctx, call(kind))
        seen[kind] = {n: round(v, 4) for n, v in by.items()}
        assert not status.any(), kind
        _, _, _, _, _, sp, op, lens = sets[kind.split("/")[0]]
        for b in (0, B // 2, B - 1):
            n = int(lens[b])
            want = torch.empty(e * n, dtype=torch.uint8, device=status.device)
            ctx.ec_encode_data(n, k, e, g, [int(p) for p in sp[b]], [want.data_ptr() + r * n for r in range(e)])
            torch.cuda.synchronize()
            got = torch.cat([row_at(sets[kind.split("/")[0]][0], int(p), n) for p in op[b]])
            assert torch.equal(got, want), (kind, b)

    def run(kind):
        ms, host = bracket(call(kind))
        wall.setdefault(kind, []).append(host)
        return ms, {}

    out = {"what": "c", "shape": {"k": k, "rows": e, "blocks": B, "skew": [big, small], "uniform_len": uni_len,
                                  "bytes_per_row_set": {"skew": int(skew.sum()), "uniform": int(uni.sum())}},
           "device": torch.cuda.get_device_name(0), "kernel_ms_of_one_run": seen,
           "runs": ml.mirrored_rounds(kinds, a.rounds, run)}
    summ = ml.summarise(out["runs"], kinds)
    for kind in kinds:
        summ[kind]["host_wall_ms_median"] = float(np.median(wall[kind]))
    for mode in ("aligned32", "default"):
        s = summ[f"skew/{mode}"]
        s["pair_ratio_to_uniform"] = pair_ratios(out["runs"], kinds, f"skew/{mode}", f"uniform/{mode}", a.rounds)
        s["minus_uniform_ms"] = s["median"] - summ[f"uniform/{mode}"]["median"]
    ml.finish(a.out, out, summ)
    ctx.close()


def row_at(buffers, ptr, n):
    """The n bytes at device address ptr, which lies in one of `buffers`."""
    for t in buffers:
        off = ptr - t.data_ptr()
        if 0 <= off and off + n <= t.numel():
            return t[off: off + n]
    raise AssertionError("address outside the arenas")


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--what", choices=("a", "b", "c"), required=True)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--blocks", type=int, default=0, help="0: the shape's own count")
    a = ap.parse_args()
    {"a": what_a, "b": what_b, "c": what_c}[a.what](a)


if __name__ == "__main__":
    main()
