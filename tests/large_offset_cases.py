"""What tests/test_gpu_large_offsets.py is built from, all of it host
arithmetic (tests/test_large_offset_cases.py checks it without a device): the
geometries whose byte offsets pass 2^31 and 2^32, numpy models of the offset
computations in csrc/ with the 32-bit mutations a one-line change would make
of them, and the periodic rows that stand in for an oracle on 4 GiB rows.

Geometries (a row is `len` bytes at `pitch`; a buffer is [B][rows] rows):
  deep   many blocks at pitch 2^20 + 64: b * rows * pitch passes 2^32 in the
         source and in the parity buffer; the pitch is no power of two, so an
         offset cut to 32 bits lands inside another block's row, not on a row
         start
  wide   two blocks at pitch 2^31 + 64 (or 2^30 + 64, 2^28 + 64 where the
         code has more rows): row * pitch and the pitch itself pass 2^31 / 2^32
  flat   the compiled (5, 4) encode on both sides of the flat tiling's guard
         (rs_bitsliced.hip launch): (2048 / len + 2) * K * pitch < 2^32
  long   one block whose rows are longer than 2^31 and than 2^32 bytes
Not a test module."""
import numpy as np

import scrub_model as sm

T31, T32 = 1 << 31, 1 << 32
MAX_LEN = T32 - 1          # include/rsgpu.h RSGPU_MAX_LEN
CAP = 24 << 30             # no test holds more device memory than this
DEEP_PITCH = (1 << 20) + 64
FILL = 0x6B                # gpu_family.DeviceBlocks fills every allocation with it
PERIOD = 6177              # odd, and no divisor of 2^31 or 2^32


# ---- deep and wide --------------------------------------------------------------

def row_offset(b, r, rows, pitch, col=0):
    """Byte offset of column `col` of row r of block b in a [B][rows] buffer."""
    return (int(b) * rows + int(r)) * int(pitch) + int(col)


def deep_blocks(e, pitch=DEEP_PITCH):
    """The fewest blocks whose parity buffer alone passes 2^32, and three more."""
    return -(-T32 // (e * pitch)) + 3


def straddler(rows, pitch):
    """The block of a [B][rows] buffer whose rows hold byte 2^32."""
    return T32 // (rows * pitch)


def special_blocks(k, e, pitch, B, extra=()):
    """Where the damage and the lists go: the first and the last block, the
    block that straddles byte 2^32 of each buffer and its two neighbours."""
    out = {0, B - 1}
    for rows in (k, e) + tuple(extra):
        if rows:
            s = straddler(rows, pitch)
            out |= {s - 1, s, s + 1}
    return sorted(b for b in out if 0 <= b < B)


def locate(addr, rows, pitch, B, L):
    """What byte `addr` of a [B][rows] buffer is: (block, row, column) when it
    is one of the first L bytes of a row (a byte the tests compare with the
    model), ("pad", block, row) when it is row padding (compared with FILL),
    None when it lies outside the buffer."""
    if not 0 <= addr < B * rows * pitch:
        return None
    row, col = divmod(addr, pitch)
    b, r = divmod(row, rows)
    return (b, r, col) if col < L else ("pad", b, r)


def cut32(x):
    """An offset computed in unsigned 32 bits."""
    return int(x) % T32


def cut31(x):
    """An offset computed in a signed int: negative from 2^31 on."""
    x = int(x) % T32
    return x - T32 if x >= T31 else x


def mutations(k, e, pitch):
    """One 32-bit mutation per kernel family, as {name: f(b, r, rows, col) ->
    byte offset the mutated code would use}.  Each is a one-line change of the
    code named; none is ever built or run."""
    return {
        # rs_update.hip and the lane kernels: (size_t)b * rows * pitch
        "block_base_u32": lambda b, r, rows, col: cut32(b * rows * pitch) + r * pitch + col,
        # rs_jit.hip / rs_kernels.hip row pointers: src + (b * rows + r) * pitch
        "row_index_u32": lambda b, r, rows, col: cut32((b * rows + r) * pitch) + col,
        # a pitch passed through an int field
        "pitch_int": lambda b, r, rows, col: (b * rows + r) * cut31(pitch) + col,
        # r * pitch as a 32-bit product beside a 64-bit block base
        "row_pitch_u32": lambda b, r, rows, col: b * rows * pitch + cut32(r * pitch) + col,
    }


# ---- the flat tiling of k_rs_bs ---------------------------------------------------

def flat_factor(L):
    return 2048 // L + 2


def flat_guard(L, K, pitch, B):
    """rs_bitsliced.hip launch(): the tiles run over the blocks' rows end to end."""
    return B > 1 and L % 2048 != 0 and L < 65536 and pitch % 32 == 0 and flat_factor(L) * K * pitch < T32


def flat_pitches(L, K):
    """The largest multiple of 32 for which the guard holds and the next one."""
    lim = T32 // (flat_factor(L) * K)          # guard: pitch < 2^32 / (factor K)
    below = lim // 32 * 32
    if flat_factor(L) * K * below >= T32:
        below -= 32
    return below, below + 32


def flat_true_edge(L, K):
    """L divides 2048: the smallest multiple of 32 at which the last lane of
    a flat tile (2048 / L - 1 blocks from the tile's first) would pass 2^32."""
    assert 2048 % L == 0
    far = (2048 // L - 1) * K
    return -(-(T32 - (L - 32)) // far) // 32 * 32 + 32


def flat_lane_offsets(L, K, pitch, B):
    """tile_pos() and run_group() of rs_bitsliced.hip for every lane of every
    flat tile: the 64-bit source offset db * K * pitch + o that the kernel
    hands to glds32 as (uint32_t), and the (block, column) it stands for."""
    tiles = (B * L + 2047) // 2048
    t0 = np.arange(tiles, dtype=np.int64)[:, None] * 2048
    lane = np.arange(64, dtype=np.int64)[None, :]
    b0 = t0 // L
    x = t0 - b0 * L + lane * 32
    db = x // L
    o = x - db * L
    inb = b0 + db < B
    off = db * K * pitch + o
    return off[inb], (b0 + db)[inb], o[inb]


# ---- long rows: periodic sources ---------------------------------------------------

def patterns(k, seed=17, p=PERIOD):
    """One random period per source row."""
    return np.random.default_rng(seed).integers(0, 256, (k, p), dtype=np.uint8)


def tile_to(pat, n, phase=0):
    """`pat` (rows, p) repeated to n bytes per row, starting at byte `phase`
    of the period."""
    p = pat.shape[-1]
    idx = (np.arange(n, dtype=np.int64) + phase) % p
    return pat[..., idx]


def parity_period(orc, c, pat):
    """The oracle's parity of one period: c (e, k), pat (k, p) -> (e, p).  The
    code is bytewise, so the parity of the tiled rows is this period tiled."""
    e, k = c.shape
    p = pat.shape[1]
    out = [np.zeros(p, np.uint8) for _ in range(e)]
    orc.encode_data(p, k, e, orc.init_tables(k, e, np.ascontiguousarray(c)),
                    [np.ascontiguousarray(r) for r in pat], out)
    return np.stack(out)


def model_parity(c, src):
    """sm-based parity of src (k, n) under c (e, k), independent of the oracle."""
    par = np.zeros((c.shape[0], src.shape[1]), np.uint8)
    for j in range(src.shape[0]):
        par ^= sm.gf_mul(c[:, j][:, None], src[j][None, :])
    return par


def chunks(n, p=PERIOD, most=1 << 30):
    """[(first byte, periods)] that cover the whole periods of an n-byte row
    in pieces of at most `most` bytes, and (first byte, bytes) of the tail."""
    per = most // p
    whole = n // p
    out = [(i * p, min(per, whole - i)) for i in range(0, whole, per)]
    return out, (whole * p, n - whole * p)
