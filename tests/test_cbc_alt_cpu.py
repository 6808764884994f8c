"""ARIA-CBC / Camellia-CBC + HMAC: everything that needs no GPU -- the model's
block function pinned to the RFCs, the model pinned to its golden file, the
argument checks of tlsrec_keytab_load_cbc and the key-block split."""
from __future__ import annotations

import ctypes
import json
import os

import numpy as np
import pytest

import mbedtls_amd as M
from mbedtls_amd import cbc as C
from tests import cbc_alt_ref as A
from tests import cbc_ref as R
from tests.prng import prng_bytes
from tests.tls12_ref import p_hash

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "cbc_alt_records.json")
MACS = [R.MAC_SHA1, R.MAC_SHA256, R.MAC_SHA384]

_K32 = bytes(range(32))
_CAM_K = bytes.fromhex("0123456789abcdeffedcba9876543210")
# (cipher, key, plaintext, ciphertext): RFC 5794 Appendix A.1 / A.3, RFC 3713 Appendix A
VECTORS = [
    (A.CIPHER_ARIA_128_CBC, _K32[:16], "00112233445566778899aabbccddeeff", "d718fbd6ab644c739da95f3be6451778"),
    (A.CIPHER_ARIA_256_CBC, _K32, "00112233445566778899aabbccddeeff", "f92bd7c79fb72e2f2b8f80c1972d24fc"),
    (A.CIPHER_CAMELLIA_128_CBC, _CAM_K, _CAM_K.hex(), "67673138549669730857065648eabe43"),
    (A.CIPHER_CAMELLIA_256_CBC, _CAM_K + bytes.fromhex("00112233445566778899aabbccddeeff"), _CAM_K.hex(),
     "9acc237dff16d76c20ef7c919e3a7509"),
]


def test_ids_and_tables():
    assert (C.CIPHER_ARIA_128_CBC, C.CIPHER_ARIA_256_CBC, C.CIPHER_CAMELLIA_128_CBC, C.CIPHER_CAMELLIA_256_CBC) == \
        (26, 27, 28, 29)
    assert C.CBC_ALT_KEYLEN == A.KEYLEN and C.CBC_ALT_MAC == A.MAC_OF
    assert not set(C.CBC_ALT_KEYLEN) & (set(M.KEYLEN) | set(C.CBC_KEYLEN))
    assert "aria-128/camellia-128-cbc" in M.version()


@pytest.mark.parametrize("cipher,key,pt,ct", VECTORS)
def test_evp_block_function_is_the_rfc_cipher(cipher, key, pt, ct):
    """one CBC block under a zero IV is the block cipher itself"""
    pt, ct = bytes.fromhex(pt), bytes.fromhex(ct)
    assert A.evp_cbc(cipher, key, bytes(16), pt, True) == ct
    assert A.evp_cbc(cipher, key, bytes(16), ct, False) == pt
    data, iv = prng_bytes(cipher, 80), prng_bytes(cipher + 100, 16)
    sealed = A.evp_cbc(cipher, key, iv, data, True)
    assert sealed != data and A.evp_cbc(cipher, key, iv, sealed, False) == data
    # chained: block i is E(p_i ^ c_(i-1))
    x = bytes(a ^ b for a, b in zip(data[16:32], sealed[:16]))
    assert A.evp_cbc(cipher, key, bytes(16), x, True) == sealed[16:32]


def test_model_swap_is_scoped():
    k = R.Key(A.CIPHER_ARIA_128_CBC, R.MAC_SHA256, 0, bytes(16), bytes(32))
    a = R.Key(R.CIPHER_AES_128_CBC, R.MAC_SHA256, 0, bytes(16), bytes(32))
    buf = bytes(16) + b"hello" + bytes(96)
    e1, e2 = A.encrypt(k, buf, 16, 5, bytes(8), 23, b"\x03\x03"), A.encrypt(a, buf, 16, 5, bytes(8), 23, b"\x03\x03")
    assert e1.status == e2.status == 0 and e1.data_len == e2.data_len and e1.buf != e2.buf
    assert e2.buf == R.encrypt(a, buf, 16, 5, bytes(8), 23, b"\x03\x03").buf
    assert R.aes_cbc is A._aes_cbc and R.encrypt is A._encrypt and R.decrypt is A._decrypt


def test_model_is_pinned_to_the_golden_records():
    G = json.load(open(GOLDEN))
    assert len(G) == 16
    seen = set()
    for g in G:
        cid = bytes.fromhex(g["cid"])
        assert g["data_len"] <= 64
        k = R.Key(g["cipher"], g["mac"], g["etm"], bytes.fromhex(g["key"]), bytes.fromhex(g["mac_key"]), cid)
        ver, ctr = bytes.fromhex(g["ver"]), bytes.fromhex(g["ctr"])
        e = A.encrypt(k, bytes.fromhex(g["plain"]), g["data_offset"], g["data_len"], ctr, g["type"], ver)
        assert (e.status, e.data_offset, e.data_len, e.type, e.cid_len) == \
            (0, g["sealed_offset"], g["sealed_len"], g["sealed_type"], len(cid))
        assert e.buf.hex() == g["sealed"]
        if not cid:
            assert e.data_len == R.record_len(g["mac"], g["etm"], g["data_len"])
        d = A.decrypt(k, e.buf, e.data_offset, e.data_len, ctr, e.type, ver, cid)
        assert (d.status, d.data_offset, d.data_len, d.type) == (0, g["opened_offset"], g["data_len"], g["type"])
        lo = g["data_offset"]
        assert d.buf[d.data_offset:d.data_offset + d.data_len] == bytes.fromhex(g["plain"])[lo:lo + g["data_len"]]
        seen.add((g["cipher"], g["mac"], g["etm"], bool(cid)))
    assert seen == {(c, m, e, x) for c, m in A.SUITES for e in (0, 1) for x in (False, True)}


class _NoTable:
    handle = None


@pytest.mark.parametrize("cipher,mac", A.SUITES)
def test_load_accepts_the_four_pairs(cipher, mac):
    """good material of a suite's pair gets as far as the missing table"""
    key, mk = bytes(32), bytes(48)
    for etm in (0, 1):
        km = C.key_material(cipher, mac, etm, key[:A.KEYLEN[cipher]], mk[:R.MACLEN[mac]])
        assert C.load_status(_NoTable(), km) == M.ERR_SSL_BAD_INPUT_DATA
    bad = C.key_material(cipher, mac, 2, key[:A.KEYLEN[cipher]], mk[:R.MACLEN[mac]])
    assert C.load_status(_NoTable(), bad) == M.ERR_SSL_BAD_INPUT_DATA
    aes = C.key_material(R.CIPHER_AES_128_CBC, R.MAC_SHA1, 0, key[:16], mk[:20])
    assert C.load_status(_NoTable(), np.concatenate([aes, C.key_material(cipher, mac, 1, key, mk)])) == \
        M.ERR_SSL_BAD_INPUT_DATA


@pytest.mark.parametrize("cipher,mac", A.SUITES)
def test_load_refuses_a_mac_outside_the_pair(cipher, mac):
    key, mk = bytes(32), bytes(48)
    ok = C.key_material(cipher, mac, 0, key, mk)
    for other in (0, 4) + tuple(m for m in MACS if m != mac):
        km = C.key_material(cipher, other, 0, key, mk)
        assert C.load_status(_NoTable(), km) == M.ERR_SSL_FEATURE_UNAVAILABLE
        assert C.load_status(_NoTable(), np.concatenate([ok, km])) == M.ERR_SSL_FEATURE_UNAVAILABLE
        # ... before tls_minor and etm are looked at
        assert C.load_status(_NoTable(), C.key_material(cipher, other, 2, key, mk, tls_minor=4)) == \
            M.ERR_SSL_FEATURE_UNAVAILABLE


def test_id_25_is_still_no_cipher():
    for mac in MACS:
        assert C.load_status(_NoTable(), C.key_material(25, mac, 0, bytes(32), bytes(48))) == \
            M.ERR_SSL_FEATURE_UNAVAILABLE
        assert C.split_key_block(25, mac, bytes(256))[0] == M.ERR_SSL_FEATURE_UNAVAILABLE
    for c in (30, 31, 32, 255):
        assert C.load_status(_NoTable(), C.key_material(c, R.MAC_SHA256, 0, bytes(32), bytes(48))) == \
            M.ERR_SSL_FEATURE_UNAVAILABLE


@pytest.mark.parametrize("cipher,mac", A.SUITES)
def test_key_block_split(cipher, mac):
    kl, ml = A.KEYLEN[cipher], R.MACLEN[mac]
    blk = p_hash("sha256", prng_bytes(3, 48), b"key expansion" + prng_bytes(4, 64), 256)
    st, cw, sw = C.split_key_block(cipher, mac, blk)
    assert st == 0
    for i, d in enumerate((cw, sw)):
        assert bytes(d["mac_key"][0]) == blk[i * ml:(i + 1) * ml] + bytes(48 - ml)
        assert bytes(d["key"][0]) == blk[2 * ml + i * kl:2 * ml + (i + 1) * kl] + bytes(32 - kl)
        assert (int(d["cipher"][0]), int(d["tls_minor"][0]), int(d["mac"][0]), int(d["etm"][0])) == (cipher, 3, mac, 0)
        assert not d["reserved"].any()
    need = 2 * ml + 2 * kl
    assert C.split_key_block(cipher, mac, blk[:need])[0] == 0
    assert C.split_key_block(cipher, mac, blk[:need - 1])[0] == M.ERR_SSL_BAD_INPUT_DATA
    for other in (m for m in MACS if m != mac):
        assert C.split_key_block(cipher, other, blk)[0] == M.ERR_SSL_FEATURE_UNAVAILABLE


@pytest.mark.parametrize("cipher,mac", A.SUITES)
def test_make_keys_argument_checks(cipher, mac):
    """judged before the PRF runs (which needs the device: tests/test_cbc_alt_gpu.py checks the keys)"""
    master, rb = prng_bytes(1, 48), prng_bytes(2, 64)
    for other in (m for m in MACS if m != mac):
        assert C.make_keys(M.tls12.PRF_SHA256, cipher, other, master, rb)[0] == M.ERR_SSL_FEATURE_UNAVAILABLE
    assert C.make_keys(M.tls12.PRF_NONE, cipher, mac, master, rb)[0] == M.ERR_SSL_FEATURE_UNAVAILABLE


def test_aead_entry_points_answer_unknown_for_the_new_ids():
    """those of include/tlsrec.h's list that judge the cipher before they need a table or the device (the rest:
    tests/test_cbc_alt_gpu.py)"""
    from mbedtls_amd import _abi, stream
    lib = M.load()
    blk, ks = (ctypes.c_ubyte * 256)(), _abi.CKeySet()
    key, iv = bytes(32), bytes(16)
    for c in sorted(A.KEYLEN):
        assert lib.tlsrec_tls12_split_key_block(c, ctypes.addressof(blk), 256, ctypes.addressof(ks)) == \
            M.ERR_SSL_FEATURE_UNAVAILABLE
        assert stream.out_size(M.VERSION_TLS1_2, c, 16, 1000) == 0
        assert lib.tlsrec_dtls_out_size(c, 16, 0, 1000, 0) == 0
        got = []
        for cipher in (c, 25, 99):                      # tlsrec_transform_setup: as an unknown cipher, same transform
            t = _abi.CTransform()
            ctypes.memset(ctypes.byref(t), 0x5a, ctypes.sizeof(t))
            r = lib.tlsrec_transform_setup(ctypes.byref(t), M.VERSION_TLS1_2, cipher, key, key, iv, iv)
            got.append((r, bytes(t)))
        assert got[0][0] == M.ERR_SSL_FEATURE_UNAVAILABLE and got[0] == got[1] == got[2]
        t = _abi.CTransform.from_buffer_copy(got[0][1])
        assert (t.slot_enc, t.slot_dec, t.keylen, t.cipher) == (-1, -1, 0, 0)
        for prf in (M.tls12.PRF_SHA256, M.tls12.PRF_SHA384):
            m, rb = (ctypes.c_ubyte * 48)(), (ctypes.c_ubyte * 64)()
            assert lib.tlsrec_tls12_make_keys(prf, c, ctypes.addressof(m), ctypes.addressof(rb),
                                              ctypes.addressof(ks)) == M.ERR_SSL_FEATURE_UNAVAILABLE
