"""C ABI v14, the mask calls and the Linear / Sum prover loops (include/rzk.h): the additions leave the
version at 14, the eight new symbols are declared in include/rzk.h, listed in the binding's table and exported by the built
library, the host and device forms take one argument list, a NULL context is an argument error, and the Python layers have the
new callables.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> number of arguments
SYMBOLS = {
    "rzk_linear_mask_batch": 8,
    "rzk_linear_mask_batch_dev": 8,
    "rzk_sum_mask_batch": 9,
    "rzk_sum_mask_batch_dev": 9,
    "rzk_linear_prove_zk_batch": 21,
    "rzk_linear_prove_zk_batch_dev": 21,
    "rzk_sum_prove_zk_batch": 22,
    "rzk_sum_prove_zk_batch_dev": 22,
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


def test_version_stays_14():
    from ring_zk_amd import _lib

    m = re.search(r"#define RZK_ABI_VERSION (\d+)u", header())
    assert m and int(m.group(1)) == 14 == _lib.ABI_VERSION


def test_new_symbols_declared_bound_and_exported(built):
    from ring_zk_amd import _lib

    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    lib = C.CDLL(built)
    assert len(SYMBOLS) == 8
    for name, nargs in SYMBOLS.items():
        args = args_of(code, name)
        assert args.count(",") + 1 == nargs, name
        assert name in _lib.SIGNATURES, f"{name} missing from _lib.SIGNATURES"
        assert _lib.SIGNATURES[name][0] is C.c_int
        assert len(_lib.SIGNATURES[name][1]) == nargs, f"{name}: argument count differs from the header"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert int(lib.rzk_abi_version()) == 14


def test_host_and_device_forms_take_one_argument_list():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in SYMBOLS:
        if not name.endswith("_dev"):
            assert args_of(code, name) == args_of(code, name + "_dev"), name
    lin, summ = args_of(code, "rzk_linear_prove_zk_batch"), args_of(code, "rzk_sum_prove_zk_batch")
    for a in (lin, summ):
        assert not re.search(r"\bint32_t\b", a)                              # 64-bit slabs only
        for piece in ("const uint8_t nonce0[16]", "uint32_t stream", "int gauss_kind", "const uint8_t* aux32", "uint32_t max_rounds",
                      "uint8_t* ok", "uint8_t* rounds", "uint32_t* rounds_run", "size_t B"):
            assert piece in a, piece
        assert len(re.findall(r"(?<!const )\bint64_t\*", a)) == 9             # nine output slabs
    assert summ.startswith("rzk_ctx* ctx, uint32_t V,") and args_of(code, "rzk_sum_mask_batch").startswith("rzk_ctx* ctx, uint32_t V,")


def test_null_context_is_an_argument_error(built):
    lib = C.CDLL(built)
    null = C.c_void_p(None)
    for name, nargs in SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype = C.c_int
        lead = [null] + ([C.c_uint32(2)] if "_sum_" in name else [])
        if "_mask_" in name:
            args = lead + [null] * 6 + [C.c_size_t(1)]
        else:
            nonce = (C.c_uint8 * 16)()
            args = lead + [null, null, nonce, C.c_uint32(0), C.c_int(0), null, C.c_uint32(4)] + [null] * 12 + [C.c_size_t(1)]
        assert len(args) == nargs, name
        assert fn(*args) == -1, name


def test_python_layers_have_the_callables():
    from ring_zk_amd import Context, fiat_shamir

    for m in ("linear_mask", "sum_mask", "linear_prove_zk", "sum_prove_zk"):
        assert callable(getattr(Context, m, None)), m
    for m in ("linear_prove_zk_native", "sum_prove_zk_native", "linear_prove_zk", "sum_prove_zk"):
        assert callable(getattr(fiat_shamir, m, None)), m
