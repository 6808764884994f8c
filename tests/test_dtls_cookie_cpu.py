"""CPU-side checks of the DTLS cookie batch: the checker of tests/cookie_ref.py
against the reference's own cookie_parsing vectors (tests/golden/
dtls_cookie.json, transcribed from its test suite), the layouts the binding
shares with include/tlsrec.h, and the loud failure without a device."""
import ctypes
import hashlib
import hmac
import json
import os
import re

import pytest

import mbedtls_amd as M
from mbedtls_amd import _abi
from tests import cookie_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "dtls_cookie.json")))["cases"]
KEY = bytes(range(32))
OUT_CONTENT_LEN = 16384          # MBEDTLS_SSL_OUT_CONTENT_LEN, the buf_len of cookie_parsing


def test_fixture_holds_the_six_reference_cases():
    assert len(CASES) == 6
    assert sorted(c["ret_name"] for c in CASES) == ["MBEDTLS_ERR_SSL_DECODE_ERROR"] * 5 + \
        ["MBEDTLS_ERR_SSL_INTERNAL_ERROR"]
    assert [c["line"] for c in CASES] == [3330, 3333, 3336, 3339, 3342, 3345]


@pytest.mark.parametrize("case", [c for c in CASES if c["ret"] == R.DECODE_ERROR], ids=lambda c: c["name"])
def test_malformed_vectors_give_decode_error(case):
    dgram = bytes.fromhex(case["datagram"])
    for out_cap in (0, 27, 28, 59, 60, OUT_CONTENT_LEN):
        assert R.check_clihlo(KEY, 60, 1000, b"\x0a\x00\x00\x01\x12\x34", dgram, out_cap) == (R.DECODE_ERROR, b"")


def test_nominal_vector():
    """the reference records INTERNAL_ERROR: its context has no cookie
    callbacks, so f_cookie_write fails -- the path a buffer of 28..59 bytes
    takes here; with room for the cookie the all-zero cookie is answered by a
    HelloVerifyRequest"""
    (case,) = [c for c in CASES if c["ret"] == R.INTERNAL_ERROR]
    dgram = bytes.fromhex(case["datagram"])
    assert len(dgram) == 93 and dgram[59] == 0 and dgram[60] == 32 and dgram[61:] == bytes(32)
    cli_id, now = b"\x0a\x00\x00\x01\x12\x34", 0x65000000
    for out_cap in range(0, 28):
        assert R.check_clihlo(KEY, 60, now, cli_id, dgram, out_cap) == (R.BUFFER_TOO_SMALL, b"")
    for out_cap in range(28, 60):
        assert R.check_clihlo(KEY, 60, now, cli_id, dgram, out_cap) == (case["ret"], b"")
    for out_cap in (60, 61, OUT_CONTENT_LEN):
        st, hvr = R.check_clihlo(KEY, 60, now, cli_id, dgram, out_cap)
        assert st == R.HELLO_VERIFY_REQUIRED and len(hvr) == 60
        mac = hmac.new(KEY, now.to_bytes(4, "big") + cli_id, hashlib.sha256).digest()[:28]
        assert hvr == (dgram[:11] + bytes([0, 47, 3, 0, 0, 35]) + dgram[17:22] + bytes([0, 0, 35, 0xfe, 0xff, 32]) +
                       now.to_bytes(4, "big") + mac)
        # the cookie of the HelloVerifyRequest, echoed, passes; another client's does not
        hello2 = dgram[:61] + hvr[28:]
        assert R.check_clihlo(KEY, 60, now + 60, cli_id, hello2, 60) == (0, b"")
        assert R.check_clihlo(KEY, 60, now + 61, cli_id, hello2, 60)[0] == R.HELLO_VERIFY_REQUIRED
        assert R.check_clihlo(KEY, 60, now, cli_id + b"x", hello2, 60)[0] == R.HELLO_VERIFY_REQUIRED


def test_model_cookie_rules():
    """the order of ssl_cookie.c:198-242 and its unsigned 64-bit age"""
    now, cid = 1 << 31, b"client"
    st, ck = R.cookie_write(KEY, now, cid, 32)
    assert st == 0 and len(ck) == 32 and ck[:4] == now.to_bytes(4, "big")
    assert R.cookie_write(KEY, now, cid, 31) == (R.BUFFER_TOO_SMALL, b"")
    assert R.cookie_check(KEY, 60, now, ck, cid)[0] == 0
    assert R.cookie_check(KEY, 60, now + 60, ck, cid)[0] == 0
    assert R.cookie_check(KEY, 60, now + 61, ck, cid)[0] == -1
    assert R.cookie_check(KEY, 60, now - 1, ck, cid)[0] == -1        # from the future
    assert R.cookie_check(KEY, 0, now - 1, ck, cid)[0] == 0
    assert R.cookie_check(KEY, 0, now + (1 << 31), ck, cid)[0] == 0
    assert R.cookie_check(KEY, 60, now, ck[:31], cid)[0] == -1
    assert R.cookie_check(KEY, 60, now + 61, ck[:31] + bytes([ck[31] ^ 1]), cid)[0] == R.INVALID_MAC
    assert R.cookie_check(KEY, 60, now, ck, b"clienT")[0] == R.INVALID_MAC


def test_layouts_and_constants():
    src = open(os.path.join(ROOT, "include", "tlsrec.h")).read()

    def define(name):
        return int(re.search(r"#define\s+%s\s+\(?(-?\w+)\)?" % name, src).group(1), 0)

    assert define("TLSREC_COOKIE_TIMEOUT") == M.COOKIE_TIMEOUT == 60
    assert define("TLSREC_COOKIE_LEN") == M.COOKIE_LEN == 32
    assert define("TLSREC_DTLS_HVR_LEN") == M.DTLS_HVR_LEN == 60
    assert define("TLSREC_ERR_SSL_DECODE_ERROR") == M.ERR_SSL_DECODE_ERROR == R.DECODE_ERROR == -0x7300
    assert define("TLSREC_ERR_SSL_HELLO_VERIFY_REQUIRED") == M.ERR_SSL_HELLO_VERIFY_REQUIRED == \
        R.HELLO_VERIFY_REQUIRED == -0x6A80
    assert (R.BAD_INPUT_DATA, R.BUFFER_TOO_SMALL, R.INVALID_MAC, R.INTERNAL_ERROR) == \
        (M.ERR_SSL_BAD_INPUT_DATA, M.ERR_SSL_BUFFER_TOO_SMALL, M.ERR_SSL_INVALID_MAC, M.ERR_SSL_INTERNAL_ERROR)
    assert M.COOKIE_ITEM.itemsize == 24 and M.CLIHLO.itemsize == 40 and M.CLIHLO_RES.itemsize == 8
    assert [M.COOKIE_ITEM.fields[f][1] for f in ("id_off", "cookie_off", "id_len", "cookie_len")] == [0, 8, 16, 20]
    assert [M.CLIHLO.fields[f][1] for f in ("off", "id_off", "out_off", "len", "id_len", "out_cap", "reserved")] == \
        [0, 8, 16, 24, 28, 32, 36]
    assert [M.CLIHLO_RES.fields[f][1] for f in ("status", "olen")] == [0, 4]
    for name in ("tlsrec_cookie_setup", "tlsrec_cookie_set_timeout", "tlsrec_cookie_free", "tlsrec_cookie_batch_write",
                 "tlsrec_cookie_batch_check", "tlsrec_cookie_write", "tlsrec_cookie_check",
                 "tlsrec_dtls_check_clihlo_cookies"):
        assert name in _abi.SIGNATURES and hasattr(M.load(), name), name


def test_host_argument_checks():
    """what the calls refuse before they look for a device"""
    L = M.load()
    assert L.tlsrec_cookie_setup(None, KEY, 60) == M.ERR_SSL_BAD_INPUT_DATA
    assert L.tlsrec_cookie_batch_write(None, 0, None, 0, None, None, None, None) == M.ERR_SSL_BAD_INPUT_DATA
    assert L.tlsrec_cookie_batch_check(None, 0, None, 0, None, None, None, None) == M.ERR_SSL_BAD_INPUT_DATA
    assert L.tlsrec_dtls_check_clihlo_cookies(None, 0, None, 0, None, None, None, None, None) == \
        M.ERR_SSL_BAD_INPUT_DATA
    p = ctypes.c_void_p(0)
    assert L.tlsrec_cookie_write(None, ctypes.byref(p), None, b"id", 2) == M.ERR_SSL_BAD_INPUT_DATA
    assert L.tlsrec_cookie_check(None, bytes(32), 32, b"id", 2) == M.ERR_SSL_BAD_INPUT_DATA
    L.tlsrec_cookie_free(None)
    L.tlsrec_cookie_set_timeout(None, 5)


def test_no_gpu_means_loud_failure():
    """Without a device the context cannot be set up: HW_ACCEL_FAILED, no CPU cookie."""
    L = M.load()
    if L.tlsrec_device_check() == 0:
        pytest.skip("a device is present")
    for key in (KEY, None):
        h = ctypes.c_void_p(1)
        assert L.tlsrec_cookie_setup(ctypes.byref(h), key, M.COOKIE_TIMEOUT) == M.ERR_SSL_HW_ACCEL_FAILED
        assert h.value is None
    with pytest.raises(RuntimeError):
        M.CookieContext(KEY)
