"""The footprint check of tests/footprint.py on the host: one byte flipped in
each forbidden region of a decode's and an encode's arena in turn must fail
the check and be named; a write to every allowed byte must pass.  This is the
proof that tests/test_gpu_footprint.py can fail; it needs no wrong kernel."""
import numpy as np
import pytest

import footprint as fp

K, E, B, L, PITCH, WS = 5, 4, 3, 40, 56, 1000


def decode_layout(offset=0, pitch=PITCH):
    lay = fp.Layout()
    lay.rows("src", B, K, pitch, L, offset)
    lay.rows("par", B, E, pitch, L, offset)
    lay.rows("out", B, E, pitch, L, offset)
    lay.flat("err", B * E)
    lay.flat("workspace", WS)
    lay.flat("status", 4 * B)
    return lay


def flipped(before, off):
    after = before.copy()
    after[off] ^= 0x01
    return after


def test_layout_alignment_and_guards():
    for offset in (0, 1, 15):
        lay = decode_layout(offset)
        prev_end = 0
        for r in lay.regions:
            want = offset if r.is_rows else 0
            assert r.start % fp.ALIGN == want and r.start - prev_end >= fp.GUARD, r.name
            prev_end = r.end
        assert lay.size - prev_end == fp.GUARD
        assert lay["out"].size == (B * E - 1) * PITCH + L


def test_noise_is_seeded_and_no_constant():
    lay = decode_layout()
    a, b = lay.noise(3), lay.noise(3)
    assert np.array_equal(a, b) and not np.array_equal(a, lay.noise(4))
    assert len(np.unique(a)) == 256


def forbidden_decode(lay):
    """(arena byte, the name check must give it) for a whole decode."""
    src, par, out, err, ws, st = (lay[n] for n in ("src", "par", "out", "err", "workspace", "status"))
    cases = [(0, "guard before src"), (src.start - 1, "guard before src")]
    for r in (src, par, out):
        cases += [(r.end, f"guard after {r.name}"), (r.end + fp.GUARD - 1, f"guard after {r.name}")]
    cases += [(lay.size - 1, "status + 4096 past its size")]
    # the first and the last byte of a row's padding: the first row's, and
    # the last row's that has padding inside the buffer
    cases += [(out.row_start(0, 0) + L, "out row (b=0, i=0) padding"),
              (out.row_start(0, 0) + PITCH - 1, "out row (b=0, i=0) padding"),
              (out.row_start(1, 3) + L, "out row (b=1, i=3) padding"),
              (out.row_start(2, 2) + PITCH - 1, "out row (b=2, i=2) padding")]
    cases += [(ws.end, "workspace + 1 past its size"), (ws.end + 16, "workspace + 17 past its size")]
    cases += [(st.end, "status + 1 past its size"), (st.end + 3, "status + 4 past its size")]
    cases += [(src.row_start(1, 2) + 7, "src row (b=1, i=2)"), (src.row_start(2, 4) + L - 1, "src row (b=2, i=4)"),
              (src.row_start(0, 1) + L, "src row (b=0, i=1) padding"),
              (par.row_start(0, 0), "par row (b=0, i=0)"), (par.row_start(2, 3) + L - 1, "par row (b=2, i=3)"),
              (err.start, "err + 0"), (err.end - 1, f"err + {B * E - 1}"), (err.end, "err + 1 past its size")]
    return cases


@pytest.mark.parametrize("offset", [0, 1])
def test_every_forbidden_region_of_a_decode_is_caught_and_named(offset):
    lay = decode_layout(offset)
    before = lay.noise(1)
    allowed = fp.decode_allowed(lay, WS)
    lay.check(before, before.copy(), allowed)
    for off, name in forbidden_decode(lay):
        with pytest.raises(AssertionError) as ei:
            lay.check(before, flipped(before, off), allowed)
        assert str(ei.value).startswith(name + ": "), (off, name, str(ei.value))


def test_every_allowed_byte_of_a_decode_may_change():
    lay = decode_layout()
    before = lay.noise(1)
    after = before.copy()
    allowed = fp.decode_allowed(lay, WS)
    n = 0
    for s, e in allowed:
        after[s:e] ^= 0xFF
        n += e - s
    assert n == B * E * L + WS + 4 * B and int((before != after).sum()) == n
    lay.check(before, after, allowed)


def test_a_declared_size_smaller_than_the_buffer():
    """The workspace may be laid out larger than the size the library
    declares: the byte right after the declared size is inside the buffer and
    still forbidden."""
    lay = decode_layout()
    before = lay.noise(2)
    allowed = fp.decode_allowed(lay, WS - 100)
    with pytest.raises(AssertionError, match=rf"^workspace \+ {WS - 100}: "):
        lay.check(before, flipped(before, lay["workspace"].start + WS - 100), allowed)
    lay.check(before, flipped(before, lay["workspace"].start + WS - 101), allowed)


def test_prepare_and_apply_footprints():
    """The prepare alone may write the workspace and the status, the apply the
    outputs: each one's bytes are forbidden to the other."""
    lay = decode_layout()
    before = lay.noise(1)
    prep = fp.decode_allowed(lay, WS, out=False)
    app = fp.decode_allowed(lay, WS, prepare=False)
    o, w, s = lay["out"].row_start(1, 1), lay["workspace"].start + 5, lay["status"].start + 4
    lay.check(before, flipped(before, w), prep)
    lay.check(before, flipped(before, s), prep)
    lay.check(before, flipped(before, o), app)
    with pytest.raises(AssertionError, match=r"^out row \(b=1, i=1\): "):
        lay.check(before, flipped(before, o), prep)
    with pytest.raises(AssertionError, match=r"^workspace \+ 5: "):
        lay.check(before, flipped(before, w), app)
    with pytest.raises(AssertionError, match=r"^status \+ 4: "):
        lay.check(before, flipped(before, s), app)


def test_fewer_blocks_than_the_arena_holds():
    """A call on the first blocks only: the rows and the statuses of the
    others are forbidden."""
    lay = decode_layout()
    before = lay.noise(1)
    allowed = fp.decode_allowed(lay, WS, blocks=2)
    with pytest.raises(AssertionError, match=r"^out row \(b=2, i=0\): "):
        lay.check(before, flipped(before, lay["out"].row_start(2, 0)), allowed)
    with pytest.raises(AssertionError, match=r"^status \+ 8: "):
        lay.check(before, flipped(before, lay["status"].start + 8), allowed)


def test_encode_footprint():
    lay = fp.Layout()
    lay.rows("src", B, K, PITCH, L, 15)
    lay.rows("par", B, E, PITCH, L, 15)
    before = lay.noise(5)
    allowed = fp.encode_allowed(lay)
    after = before.copy()
    for s, e in allowed:
        after[s:e] ^= 0xFF
    lay.check(before, after, allowed)
    par, src = lay["par"], lay["src"]
    for off, name in [(0, "guard before src"), (src.start, "src row (b=0, i=0)"), (src.end - 1, "src row (b=2, i=4)"),
                      (src.end, "guard after src"), (par.start - 1, "guard after src"),
                      (par.row_start(0, 0) + L, "par row (b=0, i=0) padding"),
                      (par.row_start(2, 2) + PITCH - 1, "par row (b=2, i=2) padding"),
                      (par.end, "guard after par"), (lay.size - 1, "guard after par")]:
        with pytest.raises(AssertionError) as ei:
            lay.check(before, flipped(before, off), allowed)
        assert str(ei.value).startswith(name + ": "), (off, name, str(ei.value))


def test_pitch_equal_to_len_has_no_padding():
    """With pitch == len a store past a row's end lands in the next row's
    [0, len), which is allowed: only the last row's overrun shows, in the
    guard."""
    lay = decode_layout(pitch=L)
    before = lay.noise(1)
    allowed = fp.decode_allowed(lay, WS)
    out = lay["out"]
    lay.check(before, flipped(before, out.row_start(0, 0) + L), allowed)
    with pytest.raises(AssertionError, match=r"^guard after out: "):
        lay.check(before, flipped(before, out.row_start(2, 3) + L), allowed)


def test_the_first_offending_byte_is_reported():
    lay = decode_layout()
    before = lay.noise(1)
    after = flipped(flipped(before, lay["out"].end + 3), lay["src"].row_start(0, 0) + 2)
    with pytest.raises(AssertionError, match=r"^src row \(b=0, i=0\): arena byte \d+ written .* 2 bytes"):
        lay.check(before, after, fp.decode_allowed(lay, WS))
