"""CPU tier of the batched message codec: the schema walk (ring_zk_amd/csrc/rzk_wire_walk.h), compiled with g++ under
-fsanitize=address,undefined into tests/wire_walk/walk_driver.cpp, against an independent Python restatement of the
serde rules (bincode, the reference's default options, src/mat.rs:424-438):

  * little-endian, a u64 count before every Vec, struct fields in declaration order without tags;
  * a Polynomial is its trimmed coefficient Vec, a Mat is Vec<Vec<Polynomial>> (every message Mat is a column);
  * an Option is a 1-byte tag (0 None, 1 Some) followed by the value.

Hand-assembled messages of every kind give the expected positions; every reject case (truncation at every byte, a
wrong count in each field, len = N+1, len = 2^63, a count near 2^64, Option tag 2, trailing bytes) gives ok = 0; a
seeded fuzz of mutated messages never reads outside the span (the sanitizer aborts the driver otherwise) and agrees
with the Python walker.  The message encoder below is also the expected-bytes source of tests/test_gpu_wire_messages.py.
"""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# ---- independent restatement of the message schemas (reference structs, fields in declaration order) ----------------
# ("mat", rows) Mat rows x 1 | ("vec", rows) Vec<Polynomial> | ("poly",) Polynomial | ("opt",) Option<Polynomial>;
# ("vmat", rows) / ("vvec", rows) wrapped in a Vec of V
COMMITMENT, OPENING, CHALLENGE, OPEN_COMMITMENT, OPEN_RESPONSE, LINEAR_COMMITMENT, SUM_COMMITMENT, SUM_RESPONSE = range(8)
KIND_NAMES = ["COMMITMENT", "OPENING", "CHALLENGE", "OPEN_COMMITMENT", "OPEN_RESPONSE", "LINEAR_COMMITMENT",
              "SUM_COMMITMENT", "SUM_RESPONSE"]


def schema(kind, n, k, l, V=1):
    """[(name, form, rows)] of a message kind: commit.rs:134,222; open.rs:190-228; linear.rs:271-315; sum.rs:342-391."""
    return {
        COMMITMENT: [("c", "mat", n + l)],
        OPENING: [("x", "vec", l), ("r", "mat", k), ("f", "opt", 1)],
        CHALLENGE: [("d", "poly", 1)],
        OPEN_COMMITMENT: [("c", "mat", n + l), ("t", "vec", n)],
        OPEN_RESPONSE: [("z", "mat", k)],
        LINEAR_COMMITMENT: [("c", "mat", n + l), ("cp", "mat", n + l), ("g", "poly", 1), ("t", "vec", n),
                            ("tp", "vec", n), ("u", "mat", l)],
        SUM_COMMITMENT: [("cp", "mat", n + l), ("cs", "vmat", n + l), ("gs", "vec", V), ("tp", "vec", n),
                         ("ts", "vvec", n), ("u", "mat", l)],
        SUM_RESPONSE: [("zp", "mat", k), ("zs", "vmat", k)],
    }[kind]


def field_shape(form, rows, V, N):
    """Slab shape of one field of one message."""
    if form in ("poly", "opt"):
        return (N,)
    if form in ("vmat", "vvec"):
        return (V, rows, N)
    return (rows, N)


def enc_poly(p, cb):
    p = np.asarray(p, dtype=np.int64)
    nz = np.flatnonzero(p)
    ln = int(nz[-1]) + 1 if nz.size else 0   # trimmed: no trailing zero coefficients
    return struct.pack("<Q", ln) + p[:ln].astype("<i8" if cb == 8 else "<i4").tobytes()


def enc_vec(polys, cb):
    return struct.pack("<Q", len(polys)) + b"".join(enc_poly(p, cb) for p in polys)


def enc_mat(rows, cb):
    return struct.pack("<Q", len(rows)) + b"".join(struct.pack("<Q", 1) + enc_poly(p, cb) for p in rows)


def encode_message(kind, fields, n, k, l, V=1, cb=8):
    """One message from its field slabs (numpy, one message's part); fields[i] None = Option None."""
    out = b""
    for (name, form, rows), a in zip(schema(kind, n, k, l, V), fields):
        if form == "mat":
            out += enc_mat(list(a), cb)
        elif form == "vec":
            out += enc_vec(list(a), cb)
        elif form == "poly":
            out += enc_poly(a, cb)
        elif form == "opt":
            out += b"\x00" if a is None else b"\x01" + enc_poly(a, cb)
        elif form == "vmat":
            out += struct.pack("<Q", len(a)) + b"".join(enc_mat(list(m), cb) for m in a)
        elif form == "vvec":
            out += struct.pack("<Q", len(a)) + b"".join(enc_vec(list(v), cb) for v in a)
    return out


NONE = 0xFFFF


def py_walk(msg, kind, N, n, k, l, V=1, cb=8):
    """(ok, [(coefficient position, len)]) of one message span; len = NONE for an Option that is None."""
    pos = 0
    ents = []

    class Reject(Exception):
        pass

    def u64():
        nonlocal pos
        if len(msg) - pos < 8:
            raise Reject
        v = struct.unpack_from("<Q", msg, pos)[0]
        pos += 8
        return v

    def expect(v):
        if u64() != v:
            raise Reject

    def poly():
        nonlocal pos
        ln = u64()
        if ln > N or len(msg) - pos < ln * cb:
            raise Reject
        ents.append((pos, ln))
        pos += ln * cb

    def vec(rows):
        expect(rows)
        for _ in range(rows):
            poly()

    def mat(rows):
        expect(rows)
        for _ in range(rows):
            expect(1)
            poly()

    try:
        for _, form, rows in schema(kind, n, k, l, V):
            if form == "mat":
                mat(rows)
            elif form == "vec":
                vec(rows)
            elif form == "poly":
                poly()
            elif form == "opt":
                if pos >= len(msg):
                    raise Reject
                tag = msg[pos]
                pos += 1
                if tag > 1:
                    raise Reject
                if tag == 0:
                    ents.append((pos, NONE))
                else:
                    poly()
            elif form == "vmat":
                expect(V)
                for _ in range(V):
                    mat(rows)
            elif form == "vvec":
                expect(V)
                for _ in range(V):
                    vec(rows)
    except Reject:
        return False, []
    return pos == len(msg), ents if pos == len(msg) else []


def random_fields(rng, kind, N, n, k, l, V, cb, none=False, lim=None):
    """Field slabs of one message with mixed trimmed lengths: full, short, sparse and zero polynomials; coefficients
    in [-lim, lim]."""
    if lim is None:
        lim = 2 ** 31 - 1 if cb == 4 else 2 ** 40
    out = []
    for name, form, rows in schema(kind, n, k, l, V):
        if form == "opt" and none:
            out.append(None)
            continue
        a = rng.integers(-lim, lim + 1, field_shape(form, rows, V, N), dtype=np.int64)
        flat = a.reshape(-1, N)
        for i in range(flat.shape[0]):
            mode = rng.integers(0, 4)
            if mode == 1:
                flat[i, rng.integers(0, N + 1):] = 0
            elif mode == 2:
                keep = rng.random(N) < 0.2
                flat[i, ~keep] = 0
            elif mode == 3:
                flat[i] = 0
        out.append(a)
    return out


# ---- driver ---------------------------------------------------------------------------------------------------------
SHAPES = [(16, 1, 3, 1, 1), (16, 2, 5, 2, 3), (4, 1, 2, 1, 2)]   # (N, n, k, l, V)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build the walker driver")
    exe = str(tmp_path_factory.mktemp("wire_walk") / "walk_driver")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Werror", "-o", exe,
                           os.path.join(HERE, "wire_walk", "walk_driver.cpp")])
    return exe


def run_driver(exe, tmp_path, kind, N, n, k, l, V, cb, msgs):
    """msgs: [(bytes, shift)]; returns (schema line ints, struct_before list, [(ok, [(pos, len)])])."""
    path = tmp_path / ("cases_%d.bin" % os.getpid())
    with open(path, "wb") as f:
        f.write(struct.pack("<8I", kind, N, n, k, l, V, cb, len(msgs)))
        for m, shift in msgs:
            f.write(struct.pack("<IQ", shift, len(m)) + m)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stderr[-4000:]
    lines = res.stdout.splitlines()
    head = [int(v) for v in lines[0].split()[1:]]
    before = [int(v) for v in lines[1].split()]
    out = []
    for line in lines[2:]:
        parts = line.split()
        ents = [tuple(int(x) for x in p.split(":")) for p in parts[1:]]
        out.append((parts[0] == "1", ents))
    assert len(out) == len(msgs)
    return head, before, out


def polys_of(kind, n, k, l, V):
    tot = 0
    for _, form, rows in schema(kind, n, k, l, V):
        tot += (V if form in ("vmat", "vvec") else 1) * rows
    return tot


def struct_total(kind, n, k, l, V):
    """Bytes of a message besides the polynomials' len prefixes and coefficients (counts, column prefixes, tag)."""
    b = 0
    for _, form, rows in schema(kind, n, k, l, V):
        b += {"mat": 8 + 8 * rows, "vec": 8, "poly": 0, "opt": 1, "vmat": 8 + V * (8 + 8 * rows),
              "vvec": 8 + 8 * V}[form]
    return b


@pytest.mark.parametrize("cb", [8, 4])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", range(8))
def test_hand_assembled_positions(driver, tmp_path, kind, shape, cb):
    N, n, k, l, V = shape
    rng = np.random.default_rng(1000 * kind + 10 * N + cb)
    msgs, want = [], []
    for none in ((False, True) if kind == OPENING else (False,)):
        for _ in range(4):
            m = encode_message(kind, random_fields(rng, kind, N, n, k, l, V, cb, none), n, k, l, V, cb)
            ok, ents = py_walk(m, kind, N, n, k, l, V, cb)
            assert ok and len(ents) == polys_of(kind, n, k, l, V)
            msgs.append((m, 0))
            want.append((True, ents))
    head, before, got = run_driver(driver, tmp_path, kind, N, n, k, l, V, cb, msgs)
    P = polys_of(kind, n, k, l, V)
    assert head == [P, struct_total(kind, n, k, l, V), struct_total(kind, n, k, l, V) + P * (8 + N * cb)]
    assert got == want
    # encoder geometry: len prefix of polynomial j = struct_before(j) + sizes of the polynomials before it
    for ok, ents in want:
        run = 0
        for j, (pos, ln) in enumerate(ents):
            rel = before[j] + run
            assert pos == (rel if ln == NONE else rel + 8), (j, pos, rel)
            run += 0 if ln == NONE else 8 + ln * cb


def count_positions(kind, n, k, l, V, cb, N, fields):
    """Byte positions of every structural u64 count of a message (field, position), recomputed from the encoder."""
    out = []
    pos = 0
    for (name, form, rows), a in zip(schema(kind, n, k, l, V), fields):
        def poly_len(p):
            return len(enc_poly(p, cb))
        if form == "mat":
            out.append((name, pos))
            pos += 8
            for p in a:
                out.append((name + ".col", pos))
                pos += 8 + poly_len(p)
        elif form == "vec":
            out.append((name, pos))
            pos += 8 + sum(poly_len(p) for p in a)
        elif form == "poly":
            pos += poly_len(a)
        elif form == "opt":
            pos += 1 + (0 if a is None else poly_len(a))
        elif form in ("vmat", "vvec"):
            out.append((name, pos))
            pos += 8
            for m in a:
                out.append((name + ".inner", pos))
                pos += 8
                for p in m:
                    if form == "vmat":
                        out.append((name + ".col", pos))
                        pos += 8
                    pos += poly_len(p)
    return out


@pytest.mark.parametrize("cb", [8, 4])
@pytest.mark.parametrize("kind", range(8))
def test_reject_cases(driver, tmp_path, kind, cb):
    N, n, k, l, V = 16, 2, 5, 2, 3
    rng = np.random.default_rng(77 + kind + cb)
    fields = random_fields(rng, kind, N, n, k, l, V, cb)
    # the first polynomial at full length, so that len prefixes can be corrupted in place
    good = encode_message(kind, fields, n, k, l, V, cb)
    assert py_walk(good, kind, N, n, k, l, V, cb)[0]
    bad = []
    for cut in range(len(good)):                         # truncation at every byte
        bad.append(good[:cut])
    bad.append(good + b"\x00")                            # trailing bytes
    bad.append(good + b"\x00" * 8)
    for name, pos in count_positions(kind, n, k, l, V, cb, N, fields):   # a wrong count in each field
        v = struct.unpack_from("<Q", good, pos)[0]
        for w in (v + 1, v - 1, 2 ** 64 - 1, 2 ** 64 - v):
            if w % 2 ** 64 != v:
                bad.append(good[:pos] + struct.pack("<Q", w % 2 ** 64) + good[pos + 8:])
    ok, ents = py_walk(good, kind, N, n, k, l, V, cb)
    for pos, ln in ents[:3]:                              # hostile len prefixes
        if ln == NONE:
            continue
        lp = pos - 8
        for w in (N + 1, 2 ** 63, 2 ** 64 - 1, 2 ** 32 + ln):
            bad.append(good[:lp] + struct.pack("<Q", w) + good[lp + 8:])
    if kind == OPENING:                                   # Option tag 2 (and 255)
        tag_pos = len(good) - len(enc_poly(fields[2], cb)) - 1
        assert good[tag_pos] == 1
        for t in (2, 255):
            bad.append(good[:tag_pos] + bytes([t]) + good[tag_pos + 1:])
    for m in bad:
        assert not py_walk(m, kind, N, n, k, l, V, cb)[0]
    _, _, got = run_driver(driver, tmp_path, kind, N, n, k, l, V, cb, [(m, 0) for m in bad])
    assert [g[0] for g in got] == [False] * len(bad)


def test_empty_and_odd_starts(driver, tmp_path):
    """An empty span is rejected without a read; an Opening may start at any byte (byte-assembled prefixes)."""
    N, n, k, l, V, cb = 16, 1, 3, 1, 1, 8
    rng = np.random.default_rng(5)
    m = encode_message(OPENING, random_fields(rng, OPENING, N, n, k, l, V, cb), n, k, l, V, cb)
    msgs = [(b"", 0), (m, 1), (m, 3), (m, 5)]
    _, _, got = run_driver(driver, tmp_path, OPENING, N, n, k, l, V, cb, msgs)
    want = py_walk(m, OPENING, N, n, k, l, V, cb)
    assert got == [(False, [])] + [want] * 3


INTERESTING = [0, 1, 2, 3, 4, 5, 15, 16, 17, 2 ** 31, 2 ** 32, 2 ** 32 + 1, 2 ** 63, 2 ** 63 + 1, 2 ** 64 - 1,
               2 ** 64 - 8]


@pytest.mark.parametrize("cb", [8, 4])
@pytest.mark.parametrize("kind", range(8))
def test_fuzz_agrees_with_python_walker(driver, tmp_path, kind, cb):
    N, n, k, l, V = 16, 2, 5, 2, 3
    rng = np.random.default_rng(4242 + 10 * kind + cb)
    base = [encode_message(kind, random_fields(rng, kind, N, n, k, l, V, cb, none=bool(i % 2)), n, k, l, V, cb)
            for i in range(8)]
    msgs = []
    for i in range(400):
        m = bytearray(base[rng.integers(0, len(base))])
        for _ in range(int(rng.integers(1, 4))):
            op = rng.integers(0, 5)
            if op == 0 and len(m):                         # flip a byte
                m[rng.integers(0, len(m))] ^= int(rng.integers(1, 256))
            elif op == 1 and len(m) >= 8:                  # overwrite an aligned u64 with an interesting value
                p = int(rng.integers(0, len(m) // 4)) * 4
                p = min(p, len(m) - 8)
                m[p:p + 8] = struct.pack("<Q", INTERESTING[rng.integers(0, len(INTERESTING))])
            elif op == 2:                                  # truncate
                del m[int(rng.integers(0, len(m) + 1)):]
            elif op == 3:                                  # extend
                m += bytes(rng.integers(0, 256, int(rng.integers(1, 17)), dtype=np.uint8))
            elif op == 4 and len(m) >= 8:                  # +-1 on an aligned u64 (counts and lens)
                p = min(int(rng.integers(0, len(m) // 8)) * 8, len(m) - 8)
                v = struct.unpack_from("<Q", m, p)[0]
                m[p:p + 8] = struct.pack("<Q", (v + (1 if rng.random() < 0.5 else -1)) % 2 ** 64)
        msgs.append((bytes(m), 0))
    msgs += [(b, 0) for b in base]
    _, _, got = run_driver(driver, tmp_path, kind, N, n, k, l, V, cb, msgs)
    want = [py_walk(m, kind, N, n, k, l, V, cb) for m, _ in msgs]
    assert got == want
    assert sum(g[0] for g in got) >= len(base)   # the unmutated messages are accepted
