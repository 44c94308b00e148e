"""The (64, 32) encode through the Karatsuba-split generated program
(rsgpu_set_encode_kernel "karatsuba": k_rs_kara, three role waves per column
tile, combined once per tile): parity byte for byte equal to the oracle's
ec_encode_data_base restatement and to the compiled kernel's on the same
buffer, pitch padding untouched, at row lengths of one lane, around one
tile, around four tiles and with partial last tiles, for every chunk
rotation and with the wave priority on and off; where the path does not
apply, or its program cannot be built, the choice behaves as AUTO."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import rsgpu  # noqa: E402
from oracle_lib import Oracle  # noqa: E402

K, E = 64, 32
# one lane; around one tile; four tiles; one lane into a fifth; the partial
# last tile of a 1e6-byte row (18 lanes); a 32000-byte row
LENGTHS = [32, 2016, 2048, 2080, 8192, 8224, 2048 * 9 + 576, 32000]
# (L, B, wide pitch): both block counts at every length, the two pitches
# (L rounded up to 256; 1 MiB) alternating
CASES = [(L, B, (i + j) % 2 == 1) for i, L in enumerate(LENGTHS) for j, B in enumerate((1, 3))]


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU test needs a HIP device"
    c = rsgpu.Context(0)
    c.set_torch_stream()
    yield c
    torch.cuda.synchronize()
    c.set_encode_kernel("auto")
    c.close()


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def hook(ctx, name, value):
    f = getattr(rsgpu.testhooks(), name)
    f.argtypes = [C.c_void_p, C.c_int]
    assert f(ctx._h, value) == 0, (name, value)


def encode(ctx, kernel, k, e, L, B, pitch, src):
    """encode_blocks with `kernel` into a buffer pre-filled with 0x5A;
    returns (parity buffer, names of the kernels recorded)."""
    par = torch.full((B * e * pitch,), 0x5A, dtype=torch.uint8, device=src.device)
    ctx.set_encode_kernel(kernel)
    ctx.timing_read()
    ctx.timing_enable(True)
    try:
        ctx.encode_blocks(k, e, L, pitch, B, src, par)
        torch.cuda.synchronize()
        names = [n for n, _, _ in ctx.timing_read()]
    finally:
        ctx.timing_enable(False)
        ctx.set_encode_kernel("auto")
    return par, names


def sources(ctx, k, L, B, pitch, seed=11):
    src = torch.empty(B * k * pitch, dtype=torch.uint8, device=torch.device("cuda", 0))
    ctx.fill_synthetic(src, B * k, L, pitch, seed, 0)
    return src


def check_oracle(orc, k, e, L, B, pitch, src, par):
    a = orc.gen_rs_matrix(k + e, k)[k:]
    tbl = orc.init_tables(k, e, a)
    s = src.view(B, k, pitch)[:, :, :L].cpu().numpy()
    pv = par.view(B, e, pitch).cpu().numpy()
    for b in range(B):
        want = [np.zeros(L, np.uint8) for _ in range(e)]
        orc.encode_data(L, k, e, tbl, list(s[b]), want)
        for i in range(e):
            assert (pv[b, i, :L] == want[i]).all(), (k, e, L, b, i)
    assert (pv[:, :, L:] == 0x5A).all(), "pitch padding written"


@pytest.mark.parametrize("L,B,wide", CASES, ids=str)
def test_karatsuba_parity(ctx, orc, L, B, wide):
    pitch = 1 << 20 if wide else (L + 255) // 256 * 256
    src = sources(ctx, K, L, B, pitch)
    par, names = encode(ctx, "karatsuba", K, E, L, B, pitch, src)
    assert names == ["k_rs_jit(encode)"], names
    check_oracle(orc, K, E, L, B, pitch, src, par)
    ref, names = encode(ctx, "compiled", K, E, L, B, pitch, src)
    assert "k_rs_jit(encode)" not in names
    assert torch.equal(par, ref)


@pytest.fixture(scope="module")
def tile_case(ctx):
    """Sources and the compiled kernel's parity at the partial-last-tile
    length, 3 blocks: the reference of the knob tests below."""
    L, B = 2048 * 9 + 576, 3
    pitch = (L + 255) // 256 * 256
    src = sources(ctx, K, L, B, pitch, seed=23)
    ref, _ = encode(ctx, "compiled", K, E, L, B, pitch, src)
    return L, B, pitch, src, ref


@pytest.mark.parametrize("ticks", [0, 1, 37, 600])
def test_karatsuba_chunk_rotation(ctx, tile_case, ticks):
    """Every chunk order the start-time rotation can pick (period 1: any of
    the 8 chunks first) accumulates the same products."""
    L, B, pitch, src, ref = tile_case
    hook(ctx, "rsgpu_internal_set_jitw_rot", ticks)
    try:
        for _ in range(3):
            par, names = encode(ctx, "karatsuba", K, E, L, B, pitch, src)
            assert names == ["k_rs_jit(encode)"] and torch.equal(par, ref)
    finally:
        hook(ctx, "rsgpu_internal_set_jitw_rot", -1)


@pytest.mark.parametrize("prio", [0, 2])
def test_karatsuba_wave_priority(ctx, tile_case, prio):
    L, B, pitch, src, ref = tile_case
    hook(ctx, "rsgpu_internal_set_jitw_prio", prio)
    try:
        par, names = encode(ctx, "karatsuba", K, E, L, B, pitch, src)
        assert names == ["k_rs_jit(encode)"] and torch.equal(par, ref)
    finally:
        hook(ctx, "rsgpu_internal_set_jitw_prio", 2)


@pytest.mark.parametrize("k,e,L", [(64, 32, 8192 + 4), (16, 4, 4096), (64, 16, 4096), (100, 20, 8192)],
                         ids=str)
def test_karatsuba_falls_back_as_auto(ctx, orc, k, e, L):
    """len % 32 != 0, or another code: the choice behaves as AUTO (the same
    kernels recorded) and the parity equals the oracle's."""
    B = 2
    pitch = (L + 255) // 256 * 256
    src = sources(ctx, k, L, B, pitch)
    par, names = encode(ctx, "karatsuba", k, e, L, B, pitch, src)
    check_oracle(orc, k, e, L, B, pitch, src, par)
    _, auto_names = encode(ctx, "auto", k, e, L, B, pitch, src)
    assert names == auto_names, (names, auto_names)


def test_karatsuba_unavailable_falls_back_as_auto(ctx, tile_case):
    """A context in which the program could not be built (the state a failed
    build leaves, set through the test hook) encodes with AUTO's other
    kernels, forced or chosen by AUTO's threshold, and leaves no error."""
    L, B, pitch, src, ref = tile_case
    hook(ctx, "rsgpu_internal_set_kara_state", -1)
    try:
        par, names = encode(ctx, "karatsuba", K, E, L, B, pitch, src)
        assert names == ["k_rs_bs(encode)"] and torch.equal(par, ref)
        min_work(ctx, 1)
        par, names = encode(ctx, "auto", K, E, L, B, pitch, src)
        assert names == ["k_rs_bs(encode)"] and torch.equal(par, ref)
    finally:
        min_work(ctx, -1)
        hook(ctx, "rsgpu_internal_set_kara_state", 0)
    par, names = encode(ctx, "karatsuba", K, E, L, B, pitch, src)
    assert names == ["k_rs_jit(encode)"] and torch.equal(par, ref)


def test_auto_small_work_stays_compiled(ctx):
    """AUTO at (64, 32), L = 8192, 3 blocks keeps k_rs_bs."""
    L, B = 8192, 3
    src = sources(ctx, K, L, B, L)
    _, names = encode(ctx, "auto", K, E, L, B, L, src)
    assert names == ["k_rs_bs(encode)"], names


def min_work(ctx, pairs):
    f = rsgpu.testhooks().rsgpu_internal_set_kara_min_work
    f.argtypes = [C.c_void_p, C.c_longlong]
    assert f(ctx._h, pairs) == 0


def test_auto_takes_karatsuba_from_the_threshold(ctx, tile_case):
    """AUTO's threshold counts (tile, block) pairs.  The library's own
     needs ~90 GB of rows to reach, so the test hook lowers it to
    this case's 10 tiles x 3 blocks: at the threshold AUTO records
    k_rs_jit(encode) and writes the compiled kernel's bytes, one pair above
    it AUTO keeps k_rs_bs."""
    L, B, pitch, src, ref = tile_case
    try:
        min_work(ctx, 10 * B)
        par, names = encode(ctx, "auto", K, E, L, B, pitch, src)
        assert names == ["k_rs_jit(encode)"] and torch.equal(par, ref)
        min_work(ctx, 10 * B + 1)
        par, names = encode(ctx, "auto", K, E, L, B, pitch, src)
        assert names == ["k_rs_bs(encode)"] and torch.equal(par, ref)
    finally:
        min_work(ctx, -1)


def test_auto_karatsuba_round_trip_poisoned(ctx):
    """encode_all through AUTO's Karatsuba path (threshold lowered to this
    shape, 10 tiles x 2 blocks), then decode_all with every erased original
    overwritten: each recovered row equals the original."""
    L, B = 2048 * 9 + 576, 2
    try:
        min_work(ctx, 10 * B)
        enc = rsgpu.GpuEncoder(K, L, E, blocks=B, seed=17, ctx=ctx)
        ctx.timing_read()
        ctx.timing_enable(True)
        enc.encode_all()
        torch.cuda.synchronize()
        assert "k_rs_jit(encode)" in [n for n, _, _ in ctx.timing_read()]
        ctx.timing_enable(False)
        dec = rsgpu.GpuDecoder(K, L, E, blocks=B, seed=17, ctx=ctx)
        src = enc.src.view(enc.B, enc.k, enc.pitch)
        saved = {}
        for b in range(B):
            for j in dec.err_host[b]:
                saved[(b, int(j))] = src[b, int(j), :L].clone()
                src[b, int(j), :L] = 0xA5
        dec.decode_all(enc)
        torch.cuda.synchronize()
        assert dec.is_complete()
        out = dec.out.view(dec.B, dec.e, dec.pitch)
        for b in range(B):
            for i, j in enumerate(dec.err_host[b]):
                assert torch.equal(out[b, i, :L], saved[(b, int(j))]), (b, i)
    finally:
        ctx.timing_enable(False)
        min_work(ctx, -1)
