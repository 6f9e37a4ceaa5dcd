"""C ABI v14, slab32 prover (include/rzk.h "slab32 prover"): the additions leave the version at 14,
the eight new symbols are declared in include/rzk.h, listed in the binding's table and exported by the built library, their
argument lists equal the siblings' up to the coefficient type, a NULL context is an argument error, and the Python layers
have the new callables.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> (number of arguments, 64-bit sibling)
SYMBOLS = {
    "rzk_sample_uniform_keyed32_dev": (6, "rzk_sample_uniform_keyed_dev"),
    "rzk_sample_gauss_keyed32_dev": (6, "rzk_sample_gauss_keyed_dev"),
    "rzk_sample_dgauss_keyed32_dev": (6, "rzk_sample_dgauss_keyed_dev"),
    "rzk_sample_challenge_keyed32_dev": (5, "rzk_sample_challenge_keyed_dev"),
    "rzk_matvec32_batch": (6, "rzk_matvec_batch"),
    "rzk_matvec32_batch_dev": (6, "rzk_matvec_batch_dev"),
    "rzk_open_response_reject32_batch": (11, "rzk_open_response_reject_batch"),
    "rzk_open_response_reject32_batch_dev": (11, "rzk_open_response_reject_batch_dev"),
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
    assert "v14, slab32 prover" in header()


def test_new_symbols_declared_bound_and_exported(built):
    from ring_zk_amd import _lib

    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    lib = C.CDLL(built)
    assert len(SYMBOLS) == 8
    for name, (nargs, _) in SYMBOLS.items():
        args = args_of(code, name)
        assert "int32_t*" in args, f"{name} takes no 32-bit slab"
        assert args.count(",") + 1 == nargs, name
        assert name in _lib.SIGNATURES, f"{name} missing from _lib.SIGNATURES"
        assert _lib.SIGNATURES[name][0] is C.c_int
        assert len(_lib.SIGNATURES[name][1]) == nargs, f"{name}: argument count differs from the header"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert int(lib.rzk_abi_version()) == 14


def test_argument_lists_equal_the_siblings_up_to_the_coefficient_type():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name, (_, sib) in SYMBOLS.items():
        a32, a64 = args_of(code, name), args_of(code, sib)
        if "response_reject32" in name:
            # y, r, d, z are int32_t slabs; coin and E stay int64_t, accept uint8_t
            assert "const int64_t* coin" in a32 and "int64_t* E" in a32 and "uint8_t* accept" in a32
            for slab in ("y", "r", "d"):
                assert "const int32_t* %s," % slab in a32, (name, slab)
            assert "int32_t* z," in a32
            assert len(re.findall(r"\bint32_t\b", a32)) == 4 and len(re.findall(r"\bint64_t\b", a32)) == 2
        else:
            assert not re.search(r"\bint64_t\b", a32), f"{name}: every slab pointer is int32_t*"
        assert re.sub(r"\bint32_t\b", "int64_t", a32) == a64, name


def test_null_context_is_an_argument_error(built):
    lib = C.CDLL(built)
    for name, (nargs, _) in SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype = C.c_int
        args = [C.c_void_p(None)] * (nargs - 1) + [C.c_size_t(1)]
        if "sample_" in name:
            args[2] = C.c_uint32(0)
            if "uniform" in name:
                args[3] = C.c_uint64(1)
            elif "dgauss" in name:
                args[3] = C.c_uint32(1)
            elif "gauss" in name:
                args[3] = C.c_double(1.0)
        if "matvec32" in name:
            args[1] = C.c_int(0)
        if "response_reject32" in name:
            args[5], args[6] = C.c_uint64(4), C.c_double(1.0)
        assert fn(*args) == -1, name


def test_python_layers_have_the_callables():
    from ring_zk_amd import Context, backend, fiat_shamir

    for m in ("sample_uniform_keyed32", "sample_gauss_keyed32", "sample_dgauss_keyed32", "sample_challenge_keyed32", "matvec32",
              "open_response_reject32"):
        assert callable(getattr(Context, m, None)), m
    for m in ("KeyedSampler32", "ExactKeyedSampler32"):
        assert isinstance(getattr(backend, m, None), type), m
    assert issubclass(backend.KeyedSampler32, backend.KeyedSampler)
    for m in ("open_prove_sampled32", "open_prove_zk32", "draw_coins32"):
        assert callable(getattr(fiat_shamir, m, None)), m
