"""C ABI v14, the Linear proof on 32-bit slabs: the fourteen new symbols are declared in
include/rzk.h, listed in the binding's table and exported by the built library; each host form and its device form share
one argument list, which is the 64-bit sibling's with int32_t slabs; the version is still 14.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rzk_linear_commit32_batch", "rzk_linear_mask32_batch", "rzk_linear_response32_batch",
       "rzk_linear_response_reject32_batch", "rzk_linear_verify32_batch", "rzk_linear_recover32_batch", "rzk_norm2_le32_batch"]
SYMBOLS = NEW + [s + "_dev" for s in NEW]
METHODS = ["linear_commit32", "linear_mask32", "linear_response32", "linear_response_reject32", "linear_verify32",
           "linear_recover32", "norm2_le32"]
FS = ["linear_prove32", "linear_verify32", "linear_short32", "linear_verify_short32", "linear_verify_packed32",
      "linear_verify_short_packed32", "linear_prove_sampled32", "linear_prove_zk32"]


@pytest.fixture(scope="module")
def built():
    from ring_zk_amd import build

    return build.build_library()


def declarations():
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rzk.h")).read(), flags=re.S)
    return {m.group(1): [" ".join(a.split()) for a in m.group(2).split(",")]
            for m in re.finditer(r"\bint\s+(rzk_\w+)\s*\(([^)]*)\)", code)}


def test_version_is_still_14(built):
    from ring_zk_amd import _lib

    m = re.search(r"#define RZK_ABI_VERSION (\d+)u", open(os.path.join(ROOT, "include", "rzk.h")).read())
    assert m and int(m.group(1)) == 14 == _lib.ABI_VERSION
    assert int(C.CDLL(built).rzk_abi_version()) == 14


def test_symbols_declared_bound_and_exported(built):
    from ring_zk_amd import _lib

    decl = declarations()
    lib = C.CDLL(built)
    assert len(SYMBOLS) == 14
    for name in SYMBOLS:
        assert name in decl, f"{name} is not declared in include/rzk.h"
        assert name in _lib.SIGNATURES, f"{name} missing from _lib.SIGNATURES"
        assert _lib.SIGNATURES[name][0] is C.c_int
        assert len(_lib.SIGNATURES[name][1]) == len(decl[name]), f"{name}: argument count differs from the header"
        assert hasattr(lib, name), f"{name} is not exported by the library"


def test_argument_lists():
    decl = declarations()
    for name in NEW:
        assert decl[name] == decl[name + "_dev"], f"{name}: host and device form differ"
        sibling = decl[name.replace("32_batch", "_batch")]
        # the sibling's list with every coefficient slab an int32_t*; the coin and E of the reject call stay int64_t
        want = [a if a in ("const int64_t* coin", "int64_t* E") else a.replace("int64_t*", "int32_t*") for a in sibling]
        assert decl[name] == want, name
        slabs = [a for a in decl[name] if "int64_t*" in a]
        assert slabs == (["const int64_t* coin", "int64_t* E"] if "reject" in name else []), name


def test_python_surface():
    from ring_zk_amd import Context, fiat_shamir

    for m in METHODS:
        assert callable(getattr(Context, m, None)), m
    for f in FS:
        assert callable(getattr(fiat_shamir, f, None)), f


def test_null_context_is_an_argument_error(built):
    decl = declarations()
    lib = C.CDLL(built)
    for name in SYMBOLS:
        fn = getattr(lib, name)
        fn.restype = C.c_int
        args = []
        for a in decl[name]:
            if "*" in a:
                args.append(C.c_void_p(None))
            elif a.startswith("double"):
                args.append(C.c_double(1.0))
            elif a.startswith("uint64_t"):
                args.append(C.c_uint64(4))
            elif a.startswith("uint32_t"):
                args.append(C.c_uint32(1))
            else:
                assert a == "size_t B", a
                args.append(C.c_size_t(1))
        assert fn(*args) == -1, name
