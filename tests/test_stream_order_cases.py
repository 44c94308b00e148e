"""Every `int rsgpu_*(rsgpu_ctx *ctx, ...)` of include/rsgpu.h has a stream
case in tests/test_gpu_stream_order.py or a stated reason not to: an entry
point added later cannot arrive without one.  Host only."""
import os
import re

import pytest

pytest.importorskip("torch")

import test_gpu_stream_order as so  # noqa: E402

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rsgpu.h")

# entry point -> why it has no case behind the gate
EXCLUDED = {
    "rsgpu_destroy": "ends the context; it waits for the context's streams by contract",
    "rsgpu_set_stream": "the move itself; every case makes it, and the sequences pin its ordering",
    "rsgpu_synchronize": "synchronises by contract",
    "rsgpu_timing_enable": "instrumentation: enqueues nothing",
    "rsgpu_timing_read": "synchronises the streams by contract",
    "rsgpu_malloc": "allocation: enqueues nothing",
    "rsgpu_free": "deallocation: enqueues nothing",
    "rsgpu_memcpy_h2d": "synchronous by contract: the host buffer is free at the return",
    "rsgpu_memcpy_d2h": "synchronous by contract: the host buffer is filled at the return",
    "rsgpu_host_alloc": "pinned allocation: enqueues nothing",
    "rsgpu_host_free": "pinned deallocation: enqueues nothing",
    "rsgpu_encode_blocks_host": "host-resident: synchronous by contract, the parity is in host memory at the return",
    "rsgpu_decode_blocks_host": "host-resident: synchronous by contract, the rows are in host memory at the return",
    "rsgpu_set_encode_kernel": "kernel setter: host state only",
    "rsgpu_set_decode_kernel": "kernel setter: host state only",
    "rsgpu_set_scrub_kernel": "kernel setter: host state only",
    "rsgpu_set_degraded_kernel": "kernel setter: host state only",
    "rsgpu_set_rebuild_kernel": "kernel setter: host state only",
    "rsgpu_set_locate_kernel": "kernel setter: host state only",
    "rsgpu_set_repair_kernel": "kernel setter: host state only",
    "rsgpu_set_correct_kernel": "kernel setter: host state only",
}


def entry_points():
    text = open(HEADER).read()
    return re.findall(r"^int\s+(rsgpu_\w+)\s*\(\s*rsgpu_ctx\s*\*\s*ctx\b", text, re.M)


def uncovered(cases):
    return sorted(set(entry_points()) - so.covered(cases) - set(EXCLUDED))


def test_the_header_is_parsed():
    names = entry_points()
    assert len(names) == len(set(names)) and len(names) >= 41
    assert {"rsgpu_encode_blocks", "rsgpu_ec_encode_data_batch", "rsgpu_update_blocks", "rsgpu_destroy"} <= set(names)


def test_every_entry_point_has_a_case_or_a_reason():
    assert uncovered(so.CASES) == []
    assert all(len(reason.split()) >= 3 for reason in EXCLUDED.values())
    assert not set(EXCLUDED) & so.covered(so.CASES), "excluded and covered at once"
    assert set(EXCLUDED) | so.covered(so.CASES) <= set(entry_points()), "a name the header does not declare"


def test_the_table_is_not_covered_once_an_entry_point_is_removed():
    for name in sorted(so.covered(so.CASES)):
        without = {i: c for i, c in so.CASES.items() if name not in c[0]}
        assert name in uncovered(without), name
    one_less = dict(list(so.CASES.items())[1:])
    assert so.covered(one_less) <= so.covered(so.CASES)


def test_every_case_has_its_pinned_records():
    assert set(so.NAMES) == set(so.CASES)
    assert set(so.CONTROLS) <= set(so.CASES)
