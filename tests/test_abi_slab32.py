"""C ABI v14, the 32-bit coefficient slabs: the header defines version 14, every new symbol is declared in include/rzk.h,
listed in the binding's table and exported by the built library, and Context has the six methods.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rzk_narrow_batch", "rzk_widen_batch", "rzk_open_commit32_batch", "rzk_open_response32_batch",
       "rzk_open_verify32_batch", "rzk_open_recover32_batch"]
SYMBOLS = NEW + [s + "_dev" for s in NEW]


@pytest.fixture(scope="module")
def built():
    from ring_zk_amd import build

    return build.build_library()


def header():
    return open(os.path.join(ROOT, "include", "rzk.h")).read()


def test_header_defines_version_14():
    from ring_zk_amd import _lib

    m = re.search(r"#define RZK_ABI_VERSION (\d+)u", header())
    assert m and int(m.group(1)) == 14 == _lib.ABI_VERSION
    assert 'marked "v14"' in header()


def test_new_symbols_declared_bound_and_exported(built):
    from ring_zk_amd import _lib

    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    lib = C.CDLL(built)
    for name in SYMBOLS:
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, code)
        assert decl, f"{name} is not declared in include/rzk.h"
        args = decl.group(1)
        assert "int32_t*" in args, f"{name} takes no 32-bit slab"
        if "open_" in name:
            assert "int64_t" not in args, f"{name}: every slab pointer of a 32-bit Open call is int32_t*"
        else:
            assert "int64_t*" in args and "size_t count" in args
        assert name in _lib.SIGNATURES, f"{name} missing from _lib.SIGNATURES"
        assert _lib.SIGNATURES[name][0] is C.c_int
        assert len(_lib.SIGNATURES[name][1]) == args.count(",") + 1, f"{name}: argument count differs from the header"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert int(lib.rzk_abi_version()) == 14


def test_context_has_the_methods():
    from ring_zk_amd import Context

    for m in ("narrow", "widen", "open_commit32", "open_response32", "open_verify32", "open_recover32"):
        assert callable(getattr(Context, m, None)), m


def test_null_context_is_an_argument_error(built):
    lib = C.CDLL(built)
    for name in SYMBOLS:
        fn = getattr(lib, name)
        fn.restype = C.c_int
        nargs = {"narrow": 4, "widen": 4, "commit32": 8, "response32": 6, "verify32": 7, "recover32": 7}[
            re.search(r"(narrow|widen|commit32|response32|verify32|recover32)", name).group(1)]
        assert fn(*([C.c_void_p(None)] * (nargs - 1) + [C.c_size_t(1)])) == -1, name
