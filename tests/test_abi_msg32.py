"""C ABI v14, slab32 messages (include/rzk.h "32-bit slabs: messages"): the additions leave the
version at 14, every new symbol is declared in include/rzk.h, listed in the binding's table and exported by the built
library, a NULL context is an argument error, and the Python layers have the new callables.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {   # name -> number of arguments
    "rzk_fs_challenge32_batch": 9,
    "rzk_packed_encode32_batch": 7,
    "rzk_packed_decode32_batch": 7,
    "rzk_eq32_batch": 6,
}
SYMBOLS = {s + suffix: n for s, n in NEW.items() for suffix in ("", "_dev")}


@pytest.fixture(scope="module")
def built():
    from ring_zk_amd import build

    return build.build_library()


def header():
    return open(os.path.join(ROOT, "include", "rzk.h")).read()


def test_version_stays_14_and_the_block_is_marked():
    from ring_zk_amd import _lib

    m = re.search(r"#define RZK_ABI_VERSION (\d+)u", header())
    assert m and int(m.group(1)) == 14 == _lib.ABI_VERSION
    assert "v14, slab32 messages" in header()


def test_new_symbols_declared_bound_and_exported(built):
    from ring_zk_amd import _lib

    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    lib = C.CDLL(built)
    for name, nargs in SYMBOLS.items():
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, code)
        assert decl, f"{name} is not declared in include/rzk.h"
        args = decl.group(1)
        assert "int32_t*" in args and "int64_t" not in args, f"{name}: every slab pointer is int32_t*"
        assert args.count(",") + 1 == nargs, name
        assert name in _lib.SIGNATURES, f"{name} missing from _lib.SIGNATURES"
        assert _lib.SIGNATURES[name][0] is C.c_int
        assert len(_lib.SIGNATURES[name][1]) == nargs, f"{name}: argument count differs from the header"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert int(lib.rzk_abi_version()) == 14
    # the siblings' argument lists differ from the new ones in the coefficient type only
    for name in SYMBOLS:
        sib = name.replace("32_batch", "_batch")
        a32 = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, code).group(1)
        a64 = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % sib, code).group(1)
        assert re.sub(r"\s+", " ", re.sub(r"\bint32_t\b", "int64_t", a32)) == re.sub(r"\s+", " ", a64), name


def test_null_context_is_an_argument_error(built):
    lib = C.CDLL(built)
    for name, nargs in SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype = C.c_int
        args = [C.c_void_p(None)] * (nargs - 1) + [C.c_size_t(1)]
        if "fs_challenge32" in name or "packed_" in name:
            args[1], args[2] = C.c_int(3), C.c_uint32(0)
        if "eq32" in name:
            args[3] = C.c_uint32(1)
        assert fn(*args) == -1, name


def test_python_layers_have_the_callables():
    from ring_zk_amd import Context, fiat_shamir, packed

    assert callable(getattr(Context, "eq32", None))
    for m in ("encode_batch32", "decode_batch32"):
        assert callable(getattr(packed, m, None)), m
    for m in ("challenge32", "open_prove32", "open_verify32", "open_short32", "open_verify_short32", "open_verify_packed32",
              "open_verify_short_packed32"):
        assert callable(getattr(fiat_shamir, m, None)), m
