"""CPU checks of the X25519 batch calls (include/tlsrec.h, mbedtls_amd/csrc/x25519.hip):
the declarations and bindings, the argument errors in their documented order
and the no-GPU return code, and the ladder of csrc/tlsrec_x25519.h run on the
CPU through tlsrec__x25519_host -- against RFC 7748's vectors, the integer
model and OpenSSL of tests/x25519_ref.py over seeded random pairs and the edge
set -- and once more in a stand-alone program under the address and
undefined-behaviour sanitizers.  No test here needs a GPU."""
import os
import re
import subprocess

import pytest

import mbedtls_amd as M
from mbedtls_amd import _abi, build as BLD
from tests import x25519_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, HW = M.ERR_SSL_BAD_INPUT_DATA, M.ERR_SSL_HW_ACCEL_FAILED
NAMES = ("tlsrec_x25519_batch_public", "tlsrec_x25519_batch_shared")


# ---- header and bindings --------------------------------------------------------------
def test_header_declares_both_calls():
    src = open(os.path.join(ROOT, "include", "tlsrec.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), n
    L = M.load()
    for n in NAMES:
        assert n in _abi.SIGNATURES and hasattr(L, n), n
    assert len(_abi.SIGNATURES[NAMES[0]][1]) == 5 and len(_abi.SIGNATURES[NAMES[1]][1]) == 8


# ---- early returns ----------------------------------------------------------------------
# made-up addresses: every call below returns before it could touch one of them
P, Q, U, K = 0x10000, 0x20000, 0x30000, 0x40000


def test_argument_errors_in_order():
    L = M.load()
    pub, sh = L.tlsrec_x25519_batch_public, L.tlsrec_x25519_batch_shared
    # a NULL array with count != 0
    assert pub(None, Q, 32, 1, None) == BAD
    assert pub(P, None, 32, 1, None) == BAD
    assert sh(None, U, 32, Q, 32, K, 1, None) == BAD
    assert sh(P, None, 32, Q, 32, K, 1, None) == BAD
    assert sh(P, U, 32, None, 32, K, 1, None) == BAD
    assert sh(P, U, 32, Q, 32, None, 1, None) == BAD         # ok cannot be skipped
    # ... wins over a short stride, which is next
    assert pub(None, Q, 31, 1, None) == BAD
    for s in (0, 1, 31):
        assert pub(P, Q, s, 1, None) == BAD
        assert sh(P, U, s, Q, 32, K, 1, None) == BAD
        assert sh(P, U, 32, Q, s, K, 1, None) == BAD
        # a short stride is refused before count == 0 is looked at
        assert pub(P, Q, s, 0, None) == BAD
        assert sh(None, None, s, None, 32, None, 0, None) == BAD
        assert sh(None, None, 32, None, s, None, 0, None) == BAD
    # count == 0: nothing to do, NULL arrays allowed, no device asked for
    assert pub(None, None, 32, 0, None) == 0
    assert pub(P, Q, 176, 0, None) == 0
    assert sh(None, None, 32, None, 32, None, 0, None) == 0
    assert sh(P, U, 33, Q, 240, K, 0, None) == 0


def test_no_gpu_means_loud_failure():
    """without a gfx950 device a well-formed call is HW_ACCEL_FAILED, never a CPU result"""
    L = M.load()
    if L.tlsrec_device_check() == 0:
        pytest.skip("a device is present")
    assert L.tlsrec_x25519_batch_public(P, Q, 32, 1, None) == HW
    assert L.tlsrec_x25519_batch_shared(P, U, 32, Q, 32, K, 1, None) == HW
    assert L.tlsrec_x25519_batch_shared(P, U, 176, Q, 240, K, 65536, None) == HW


# ---- the ladder on the CPU, against the RFC -------------------------------------------
def test_rfc7748_section_5_2_vectors():
    for k, u, want in R.RFC_5_2:
        assert _abi.x25519_host(k, u) == (want, 1)
        assert R.model(k, u) == want


def test_rfc7748_section_6_1_exchange():
    assert _abi.x25519_host(R.ALICE_PRIV, R.BASE) == (R.ALICE_PUB, 1)
    assert _abi.x25519_host(R.BOB_PRIV, R.BASE) == (R.BOB_PUB, 1)
    assert _abi.x25519_host(R.ALICE_PRIV, R.BOB_PUB) == (R.SHARED, 1)
    assert _abi.x25519_host(R.BOB_PRIV, R.ALICE_PUB) == (R.SHARED, 1)


def test_rfc7748_iterated_vector():
    k = u = R.BASE
    for it in range(1, 1001):
        r, ok = _abi.x25519_host(k, u)
        assert ok == 1
        k, u = r, k
        if it == 1:
            assert k == R.ITER_1
    assert k == R.ITER_1000


# ---- against the model and OpenSSL ----------------------------------------------------------
def test_random_pairs_against_model_and_openssl():
    have = R.lib() is not None
    for k, u in R.random_pairs(0x7115EC0DE, 2000):
        want = R.model(k, u)
        assert _abi.x25519_host(k, u) == (want, R.ok_of(want)), (k.hex(), u.hex())
        if have:
            assert R.openssl(k, u) == want, (k.hex(), u.hex())


def test_edge_set():
    """edge scalars x edge points; ok == 0 exactly where the model's output is zero"""
    have = R.lib() is not None
    zeros = 0
    for k, u in R.edge_pairs():
        want = R.model(k, u)
        zeros += want == bytes(32)
        assert _abi.x25519_host(k, u) == (want, R.ok_of(want)), (k.hex(), u.hex())
        if have:
            assert R.openssl(k, u) == want, (k.hex(), u.hex())
    # 0, 1, p - 1, p, p + 1 and the two order-8 points, with and without bit 255, under every scalar
    assert zeros >= 14 * (len(R.EDGE_SCALARS) + 1)
    # 2^255 - 1 = p + 18 and 2^255 - 20 = p - 1: non-canonical values reduce, bit 255 is masked
    k = R.ALICE_PRIV
    assert _abi.x25519_host(k, (2 ** 255 - 1).to_bytes(32, "little"))[0] == R.model(k, (18).to_bytes(32, "little"))
    assert _abi.x25519_host(k, (9 | 1 << 255).to_bytes(32, "little"))[0] == R.ALICE_PUB
    for lo in R.LOW_ORDER:
        assert _abi.x25519_host(k, lo) == (bytes(32), 0)


def test_public_values_match_openssl():
    if R.lib() is None:
        pytest.skip("no libcrypto")
    for k, _ in R.random_pairs(0x25519A, 200):
        assert _abi.x25519_host(k, R.BASE)[0] == R.openssl_public(k)


# ---- the stand-alone program under the sanitizers --------------------------------------------
def test_host_program_under_sanitizers(tmp_path):
    """tests/c/x25519_host.cpp: the header alone, compiled for the host with the address and
    undefined-behaviour sanitizers, over the RFC vectors and the edge set.  Nothing is preloaded
    and nothing of it is loaded into this process."""
    exe, cases = str(tmp_path / "x25519_host"), str(tmp_path / "cases.txt")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    cmd = [BLD.HIPCC, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"]
    for f in san:
        cmd += ["-Xarch_host", f]
    cmd += ["-I" + BLD.CSRC, "-o", exe, os.path.join(ROOT, "tests", "c", "x25519_host.cpp"), san[0]]
    subprocess.run(cmd, check=True)
    pairs = R.edge_pairs() + R.random_pairs(0x5A17, 64)
    with open(cases, "w") as f:
        for k, u in pairs:
            want = R.model(k, u)
            f.write(f"{k.hex()} {u.hex()} {want.hex()} {R.ok_of(want)}\n")
    r = subprocess.run([exe, cases], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(pairs)} file cases" in r.stdout
