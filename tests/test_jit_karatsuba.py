"""The Karatsuba-split program of the (64, 32) encode (storage-benchmarks_amd/
csrc/jit_prog.h build_karatsuba_code, run by k_rs_kara) checked on the CPU:
the role matrices cP / cQ1 / cQ2 with rho and sigma must reproduce the
oracle's gf_gen_rs_matrix(96, 64) parity rows, and the emitted code of all
three roles -- virtual-source preamble and combine chunk included --
interpreted on a random 64-row lane image must give the oracle's 32 parity
rows, with only the allowed instructions, only registers of the Wide<16>
contract, every register read after its LDS load was waited for, and every
ds_read inside the chunk buffers."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

from oracle_lib import Oracle
from test_jit import ALLOWED, LLVM_MC, disasm, g, planes, run_chunk, unplanes

pytestmark = pytest.mark.skipif(not os.path.exists(LLVM_MC), reason="llvm-mc not available")

K, E = 64, 32
PAIRS, SRC_CHUNKS = 4, 8          # rs_jit.h kKaraPairs, kKaraSrcChunks
CHUNKS = SRC_CHUNKS + 1           # + the combine chunk
CHUNK_BUF = 2 * PAIRS * 2048      # one chunk buffer of a tile: 8 sources


def kara_source(ch, t):
    """rs_jit.h kara_source: the real source at LDS position t of chunk ch."""
    s = PAIRS * ch + t // 2
    return 32 * (s // 16) + s % 16 + 16 * (t & 1)


def karatsuba_code(coef):
    import rsgpu
    f = rsgpu.testhooks().rsgpu_internal_jit_karatsuba_code
    f.restype = C.c_longlong
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.c_void_p]
    coef = np.ascontiguousarray(coef, np.uint8)
    stride = C.c_int()
    mats = np.zeros(1584, np.uint8)
    need = f(coef.ctypes.data, None, 0, C.byref(stride), mats.ctypes.data)
    if need < 0:
        return None
    out = np.zeros(need, np.uint8)
    assert f(coef.ctypes.data, out.ctypes.data, need, C.byref(stride), mats.ctypes.data) == need
    return {"code": out.tobytes(), "stride": stride.value,
            "cP": mats[0:512].reshape(16, 32), "cQ1": mats[512:1024].reshape(16, 32),
            "cQ2": mats[1024:1536].reshape(16, 32), "rho": mats[1536:1568], "sigma": mats[1568:1584]}


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def matrix(orc):
    return orc.gen_rs_matrix(K + E, K)[K:]


@pytest.fixture(scope="module")
def prog(matrix):
    p = karatsuba_code(matrix)
    assert p is not None
    return p


def oracle_parity(orc, matrix, rows, n):
    want = [np.zeros(n, np.uint8) for _ in range(E)]
    orc.encode_data(n, K, E, orc.init_tables(K, E, matrix), [np.array(r, np.uint8) for r in rows], want)
    return [list(map(int, w)) for w in want]


def vmul(c, x):
    return [g.gf_mul(int(c), v) for v in x]


def vadd(x, y):
    return [a ^ b for a, b in zip(x, y)]


def matvec(M, xs):
    out = []
    for row in M:
        acc = [0] * len(xs[0])
        for c, x in zip(row, xs):
            acc = vadd(acc, vmul(c, x))
        out.append(acc)
    return out


def test_role_matrices_reproduce_the_code(orc, matrix, prog):
    """y[r] = P[r] ^ Q1[r], y[16 + r] = sigma_r P[r] ^ Q2[r] with P over the
    virtual sources x[base + q] ^ rho_s x[base + 16 + q], on random bytes,
    against the oracle's encode with gf_gen_rs_matrix(96, 64)."""
    rng = random.Random(64032)
    n = 32
    x = [[rng.randrange(256) for _ in range(n)] for _ in range(K)]
    xa = [x[base + q] for base in (0, 32) for q in range(16)]
    xb = [x[base + 16 + q] for base in (0, 32) for q in range(16)]
    v = [vadd(a, vmul(prog["rho"][s], b)) for s, (a, b) in enumerate(zip(xa, xb))]
    P, Q1, Q2 = matvec(prog["cP"], v), matvec(prog["cQ1"], xa), matvec(prog["cQ2"], xb)
    y = [vadd(p, q) for p, q in zip(P, Q1)]
    y += [vadd(vmul(prog["sigma"][r], P[r]), Q2[r]) for r in range(16)]
    assert y == oracle_parity(orc, matrix, x, n)


def test_other_matrices_are_refused(orc, matrix):
    """The split is checked coefficient by coefficient against the matrix it
    is built for: one changed coefficient, or a Cauchy matrix, builds nothing."""
    m = matrix.copy()
    m[17, 40] ^= 1
    assert karatsuba_code(m) is None
    assert karatsuba_code(orc.gen_cauchy1_matrix(K + E, K)[K:]) is None


def chunk_ins(prog, role, ch):
    base = (role * CHUNKS + ch) * prog["stride"]
    ins = disasm(prog["code"][base:base + prog["stride"]])
    end = next(off for off, m, _ in ins if m == "s_setpc_b64")
    return [x for x in ins if x[0] <= end]


def check_words(ins, lds_bytes):
    """Registers of the Wide<16> contract only (v9 the address, v10..v39
    planes / composites / temporaries, v40..v167 accumulators), and every
    ds_read_b128 inside the first lds_bytes of the tile's buffers, on a
    plane-half boundary."""
    for _, mnem, ops in ins:
        assert mnem in ALLOWED, mnem
        used = [int(n) for n in re.findall(r"v\[?(\d+)", ops)]
        used += [int(n) for n in re.findall(r"v\[\d+:(\d+)\]", ops)]
        assert all(9 <= r < 40 + 8 * 16 for r in used), ops
        assert "s[" not in ops or mnem == "s_setpc_b64", ops
        if mnem == "ds_read_b128":
            dst, addr = [a.strip() for a in ops.split(",")]
            m = re.fullmatch(r"v9(?: offset:(\d+))?", addr)
            assert m, ops
            off = int(m.group(1) or 0)
            assert off % 1024 == 0 and off + 1024 <= lds_bytes, ops
            lo, hi = map(int, re.fullmatch(r"v\[(\d+):(\d+)\]", dst).groups())
            assert 10 <= lo and hi < 40, "LDS loads land in planes / composites only"
        elif mnem != "s_setpc_b64" and mnem.startswith("v_"):
            assert int(re.match(r"v(\d+)", ops).group(1)) >= 10, "v9 (the LDS address) is never written"


def test_interpreted_program_encodes(orc, matrix, prog):
    """All three roles' code on one lane's 32 bytes of 64 random rows: the
    source chunks in any order leave P, Q1, Q2 in the accumulators; P's rows,
    laid out as planes where the kernel writes them, feed the combine chunks;
    Q1's slots are then parity rows 0-15 and Q2's rows 16-31 of the oracle."""
    assert prog["stride"] % 64 == 0 and len(prog["code"]) == 3 * CHUNKS * prog["stride"]
    rng = random.Random(1632)
    src = [[rng.randrange(256) for _ in range(32)] for _ in range(K)]
    want = oracle_parity(orc, matrix, src, 32)
    order = list(range(SRC_CHUNKS))
    rng.shuffle(order)  # the kernel rotates the chunk order
    regs = []
    for role in range(3):
        r = {i: 0 for i in range(256)}
        pending = []
        for ch in order:
            ins = chunk_ins(prog, role, ch)
            check_words(ins, CHUNK_BUF)
            lds = {}
            for t in range(2 * PAIRS):
                pl = planes(src[kara_source(ch, t)])
                for a in range(8):
                    lds[t * 2048 + (a // 4) * 1024 + 4 * (a % 4)] = pl[a]
            run_chunk(ins, r, lds, pending, addr_reg="v9")
            assert not pending, "a load left outstanding at the return"
        regs.append(r)
    # role P: its pure product, and a combine chunk that is a bare return
    v = [vadd(src[kara_source(s // PAIRS, 2 * (s % PAIRS))],
              vmul(prog["rho"][s], src[kara_source(s // PAIRS, 2 * (s % PAIRS) + 1)])) for s in range(32)]
    assert [unplanes([regs[0][40 + 8 * r + b] for b in range(8)]) for r in range(16)] == matvec(prog["cP"], v)
    assert chunk_ins(prog, 0, SRC_CHUNKS)[0][1] == "s_setpc_b64"
    # P's row r as planes at position r of the tile's two chunk buffers
    lds = {}
    for r in range(16):
        for a in range(8):
            lds[r * 2048 + (a // 4) * 1024 + 4 * (a % 4)] = regs[0][40 + 8 * r + a]
    for role in (1, 2):
        ins = chunk_ins(prog, role, SRC_CHUNKS)
        check_words(ins, 2 * CHUNK_BUF)
        pending = []
        run_chunk(ins, regs[role], lds, pending, addr_reg="v9")
        assert not pending
        for r in range(16):
            got = unplanes([regs[role][40 + 8 * r + b] for b in range(8)])
            assert got == want[16 * (role - 1) + r], (role, r)


def test_program_size_matches_the_priced_count(prog):
    """The VALU instructions of one tile's program (all chunks of all roles)
    stay within 3 % of tools/karatsuba_price.py's karatsuba3() before
    transposes: 5139 + 4753 + 4882 = 14774 (the C++ and Python greedy
    programs may break ties differently)."""
    n = 0
    for role in range(3):
        for ch in range(CHUNKS):
            n += sum(1 for _, m, _ in chunk_ins(prog, role, ch) if m.startswith("v_"))
    assert abs(n - 14774) <= 0.03 * 14774, n
