"""C ABI v14, prover loop (include/rzk.h "prover loop"): the additions leave the version at 14, the five
new symbols are declared in include/rzk.h, listed in the binding's table and exported by the built library, the two widths
have one argument list up to the coefficient type, a NULL context is an argument error, the Python layers have the new
callables, and KeyedSampler.take_nonces advances and overflows as _next_nonce does.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> number of arguments
SYMBOLS = {
    "rzk_open_prove_zk_batch": 15,
    "rzk_open_prove_zk_batch_dev": 15,
    "rzk_open_prove_zk32_batch": 15,
    "rzk_open_prove_zk32_batch_dev": 15,
    "rzk_debug_compact_dev": 6,
}


@pytest.fixture(scope="module")
def built():
    from ring_zk_amd import build

    return build.build_library()


def header():
    return open(os.path.join(ROOT, "include", "rzk.h")).read()


def args_of(code, name):
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, code)
    assert decl, f"{name} is not declared in include/rzk.h"
    return re.sub(r"\s+", " ", decl.group(1)).strip()


def test_version_stays_14_and_the_block_is_marked():
    from ring_zk_amd import _lib

    m = re.search(r"#define RZK_ABI_VERSION (\d+)u", header())
    assert m and int(m.group(1)) == 14 == _lib.ABI_VERSION
    assert "v14, prover loop" in header()


def test_new_symbols_declared_bound_and_exported(built):
    from ring_zk_amd import _lib

    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    lib = C.CDLL(built)
    assert len(SYMBOLS) == 5
    for name, nargs in SYMBOLS.items():
        args = args_of(code, name)
        assert args.count(",") + 1 == nargs, name
        assert name in _lib.SIGNATURES, f"{name} missing from _lib.SIGNATURES"
        assert _lib.SIGNATURES[name][0] is C.c_int
        assert len(_lib.SIGNATURES[name][1]) == nargs, f"{name}: argument count differs from the header"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert int(lib.rzk_abi_version()) == 14


def test_the_two_widths_have_one_argument_list():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for suffix in ("", "_dev"):
        a64, a32 = args_of(code, "rzk_open_prove_zk_batch" + suffix), args_of(code, "rzk_open_prove_zk32_batch" + suffix)
        assert not re.search(r"\bint64_t\b", a32) and not re.search(r"\bint32_t\b", a64)
        assert re.sub(r"\bint32_t\b", "int64_t", a32) == a64
        assert len(re.findall(r"\bint32_t\b", a32)) == 5                     # x, c, t, z, r
        for piece in ("const uint8_t nonce0[16]", "uint32_t stream", "int gauss_kind", "const uint8_t* aux32", "uint32_t max_rounds",
                      "uint8_t* ok", "uint8_t* rounds", "uint32_t* rounds_run", "size_t B"):
            assert piece in a64, piece
        assert args_of(code, "rzk_open_prove_zk_batch") == a64               # host and device forms take the same list


def test_null_context_is_an_argument_error(built):
    lib = C.CDLL(built)
    for name, nargs in SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype = C.c_int
        if name == "rzk_debug_compact_dev":
            args = [C.c_void_p(None), C.c_void_p(None), C.c_void_p(None), C.c_size_t(1), C.c_void_p(None), C.c_void_p(None)]
        else:
            nonce = (C.c_uint8 * 16)()
            args = [C.c_void_p(None), C.c_void_p(None), nonce, C.c_uint32(0), C.c_int(0), C.c_void_p(None), C.c_uint32(4)]
            args += [C.c_void_p(None)] * 7 + [C.c_size_t(1)]
        assert len(args) == nargs
        assert fn(*args) == -1, name


def test_python_layers_have_the_callables():
    from ring_zk_amd import Context, backend, fiat_shamir

    for m in ("open_prove_zk", "open_prove_zk32", "debug_compact"):
        assert callable(getattr(Context, m, None)), m
    assert callable(getattr(backend.KeyedSampler, "take_nonces", None))
    assert callable(getattr(fiat_shamir, "open_prove_zk_native", None))
    assert backend.KeyedSampler.GAUSS_KIND == 0 and backend.KeyedSampler32.GAUSS_KIND == 0
    assert backend.ExactKeyedSampler.GAUSS_KIND == 1 and backend.ExactKeyedSampler32.GAUSS_KIND == 1


class _NoDevice:
    """what KeyedSampler needs of a context, without a GPU"""

    def set_sampler_key(self, key):
        self.key = key


def test_take_nonces_advances_and_overflows_as_next_nonce():
    from ring_zk_amd.backend import KeyedSampler

    s = KeyedSampler(_NoDevice(), bytes(32), nonce0=(1 << 64) - 2)
    assert s.take_nonces(5) == ((1 << 64) - 2).to_bytes(16, "little") and s.counter == (1 << 64) + 3
    assert s._next_nonce() == ((1 << 64) + 3).to_bytes(16, "little")          # the next draw follows the nonces taken
    assert s.take_nonces(0) == ((1 << 64) + 4).to_bytes(16, "little") and s.counter == (1 << 64) + 4
    with pytest.raises(ValueError):
        s.take_nonces(-1)
    top = (1 << 128) - 4
    s = KeyedSampler(_NoDevice(), bytes(32), nonce0=top)
    with pytest.raises(OverflowError):
        s.take_nonces(5)                                                      # the fifth nonce would be 2^128
    assert s.counter == top                                                   # a refused request takes nothing
    assert s.take_nonces(4) == top.to_bytes(16, "little") and s.counter == 1 << 128
    with pytest.raises(OverflowError):
        s.take_nonces(1)
    with pytest.raises(OverflowError):
        s._next_nonce()                                                       # the existing rule, at the same counter
    ref = KeyedSampler(_NoDevice(), bytes(32), nonce0=top)
    for _ in range(4):
        ref._next_nonce()
    assert ref.counter == s.counter
