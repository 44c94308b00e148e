"""rsgpu_set_repair_kernel on the CPU (include/rsgpu.h): the symbol is exported,
declared and bound, the choices of the wrapper and of the header agree, and a
value the call does not know is refused -- a null context with every value by
the library, an unknown name by the wrapper before the library is called.
tests/test_gpu_repair_generated.py runs the kernels and refuses unknown values
on a live context."""
import ctypes as C
import os
import re
import types

import pytest

import rsgpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rsgpu.h")


def test_the_wrapper_s_choices():
    assert rsgpu.REPAIR_KERNELS == {"auto": 0, "generated": 1}
    assert "REPAIR_KERNELS" in rsgpu.__all__
    assert "rsgpu_set_repair_kernel" in rsgpu.EXPORTED_SYMBOLS
    assert callable(rsgpu.Context.set_repair_kernel)


def test_the_header_s_constants_and_declaration():
    txt = open(HEADER).read()
    got = dict(re.findall(r"^#define RSGPU_REPAIR_KERNEL_(AUTO|GENERATED)\s+(\d+)\s*$", txt, re.M))
    assert {k.lower(): int(v) for k, v in got.items()} == rsgpu.REPAIR_KERNELS
    assert re.search(r"^int rsgpu_set_repair_kernel\(rsgpu_ctx \*ctx, int kernel\);", txt, re.M)
    # the repair's modes keep their own names and values
    assert dict(re.findall(r"^#define RSGPU_REPAIR_(ONE_ROW|COLUMNS)\s+(\d+)", txt, re.M)) == {"ONE_ROW": "0",
                                                                                              "COLUMNS": "1"}


def test_the_symbol_is_exported_and_bound():
    fn = rsgpu.lib().rsgpu_set_repair_kernel
    assert fn.restype is C.c_int and fn.argtypes == [C.c_void_p, C.c_int]
    raw = C.CDLL(rsgpu.LIB_PATH)
    assert hasattr(raw, "rsgpu_set_repair_kernel")


def test_null_context_is_an_argument_error():
    for kernel in (0, 1, 2, -1):
        assert rsgpu.lib().rsgpu_set_repair_kernel(None, kernel) == -1


def test_an_unknown_name_is_refused_by_the_wrapper():
    calls = []
    stub = types.SimpleNamespace(_h=None, check=lambda rc, what: calls.append((rc, what)))
    for name in ("fused", "two_pass", "nonsense", 1):
        with pytest.raises(KeyError):
            rsgpu.Context.set_repair_kernel(stub, name)
    assert calls == []
