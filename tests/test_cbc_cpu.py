"""AES-CBC + HMAC: everything that needs no GPU -- the host helpers of
include/tlsrec.h against tests/cbc_ref.py, the key-block split, the argument
checks of tlsrec_keytab_load_cbc, and the model pinned to its golden file."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

import mbedtls_amd as M
from mbedtls_amd import cbc as C
from tests import cbc_ref as R
from tests.prng import prng_bytes
from tests.tls12_ref import p_hash

MACS = [R.MAC_SHA1, R.MAC_SHA256, R.MAC_SHA384]
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "cbc_records.json")


def test_tables_and_layout():
    assert C.CBC_KEY_MATERIAL.itemsize == 128
    assert C.CBC_KEYLEN == R.KEYLEN and C.MACLEN == R.MACLEN
    assert not set(C.CBC_KEYLEN) & set(M.KEYLEN)      # KEYLEN / TAGLEN stay the AEAD ids
    assert "cbc" in M.version()


@pytest.mark.parametrize("mac", MACS)
@pytest.mark.parametrize("etm", [0, 1])
def test_record_len_matches_the_model(mac, etm):
    for n in range(16385):
        assert C.record_len(mac, etm, n) == R.record_len(mac, etm, n), n


def test_record_len_and_minlen_unknown_ids():
    for mac, etm in ((0, 0), (4, 1), (R.MAC_SHA256, 2), (R.MAC_SHA256, -1)):
        assert C.record_len(mac, etm, 100) == 0 and C.minlen(mac, etm) == 0


def test_minlen():
    want = {(R.MAC_SHA1, 0): 48, (R.MAC_SHA1, 1): 52, (R.MAC_SHA256, 0): 64, (R.MAC_SHA256, 1): 64,
            (R.MAC_SHA384, 0): 80, (R.MAC_SHA384, 1): 80}           # ssl_tls.c:7822-7835 by hand
    for (mac, etm), v in want.items():
        assert C.minlen(mac, etm) == v == R.minlen(mac, etm)


@pytest.mark.parametrize("cipher", sorted(R.KEYLEN))
@pytest.mark.parametrize("mac", MACS)
def test_key_block_split(cipher, mac):
    kl, ml = R.KEYLEN[cipher], R.MACLEN[mac]
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
    assert C.split_key_block(cipher, mac, b"")[0] == M.ERR_SSL_BAD_INPUT_DATA


def test_key_block_split_unknown_ids():
    blk = bytes(256)
    for cipher, mac in ((M.CIPHER_AES_128_GCM, R.MAC_SHA256), (22, R.MAC_SHA1), (25, R.MAC_SHA1),
                        (R.CIPHER_AES_128_CBC, 0), (R.CIPHER_AES_256_CBC, 4)):
        assert C.split_key_block(cipher, mac, blk)[0] == M.ERR_SSL_FEATURE_UNAVAILABLE
    assert C.make_keys(M.tls12.PRF_NONE, R.CIPHER_AES_128_CBC, R.MAC_SHA1, bytes(48), bytes(64))[0] == \
        M.ERR_SSL_FEATURE_UNAVAILABLE
    assert C.make_keys(M.tls12.PRF_SHA256, 5, R.MAC_SHA1, bytes(48), bytes(64))[0] == M.ERR_SSL_FEATURE_UNAVAILABLE


def test_aead_entry_points_keep_answering_unknown_for_cbc_ids():
    import ctypes
    from mbedtls_amd import _abi, stream
    blk, ks = (ctypes.c_ubyte * 256)(), _abi.CKeySet()
    for c in (C.CIPHER_AES_128_CBC, C.CIPHER_AES_256_CBC):
        assert M.load().tlsrec_tls12_split_key_block(c, ctypes.addressof(blk), 256, ctypes.addressof(ks)) == \
            M.ERR_SSL_FEATURE_UNAVAILABLE
        assert stream.out_size(M.VERSION_TLS1_2, c, 16, 1000) == 0
        assert M.load().tlsrec_dtls_out_size(c, 16, 0, 1000, 0) == 0


class _NoTable:
    handle = None


def test_load_argument_checks_without_a_gpu():
    """host material is judged before the table or the device is touched"""
    key, mk = bytes(32), bytes(48)
    ok = C.key_material(R.CIPHER_AES_128_CBC, R.MAC_SHA256, 0, key[:16], mk[:32])
    cases = [(C.key_material(M.CIPHER_AES_128_GCM, R.MAC_SHA256, 0, key[:16], mk[:32]), M.ERR_SSL_FEATURE_UNAVAILABLE),
             (C.key_material(25, R.MAC_SHA256, 0, key[:16], mk[:32]), M.ERR_SSL_FEATURE_UNAVAILABLE),
             (C.key_material(R.CIPHER_AES_256_CBC, 0, 0, key, mk[:32]), M.ERR_SSL_FEATURE_UNAVAILABLE),
             (C.key_material(R.CIPHER_AES_256_CBC, 4, 1, key, mk[:32]), M.ERR_SSL_FEATURE_UNAVAILABLE),
             (C.key_material(R.CIPHER_AES_128_CBC, R.MAC_SHA1, 0, key[:16], mk[:20], tls_minor=4), M.ERR_SSL_BAD_INPUT_DATA),
             (C.key_material(R.CIPHER_AES_128_CBC, R.MAC_SHA1, 0, key[:16], mk[:20], tls_minor=2), M.ERR_SSL_BAD_INPUT_DATA),
             (C.key_material(R.CIPHER_AES_128_CBC, R.MAC_SHA384, 2, key[:16], mk), M.ERR_SSL_BAD_INPUT_DATA),
             (ok, M.ERR_SSL_BAD_INPUT_DATA)]              # good material, no table
    for km, want in cases:
        assert C.load_status(_NoTable(), km) == want
        both = np.concatenate([ok, km])                   # ... and as the second of two
        assert C.load_status(_NoTable(), both) == want


def test_model_is_pinned_to_the_golden_records():
    G = json.load(open(GOLDEN))
    assert len(G) == 24
    seen = set()
    for g in G:
        cid = bytes.fromhex(g["cid"])
        k = R.Key(g["cipher"], g["mac"], g["etm"], bytes.fromhex(g["key"]), bytes.fromhex(g["mac_key"]), cid)
        ver, ctr = bytes.fromhex(g["ver"]), bytes.fromhex(g["ctr"])
        e = R.encrypt(k, bytes.fromhex(g["plain"]), g["data_offset"], g["data_len"], ctr, g["type"], ver)
        assert (e.status, e.data_offset, e.data_len, e.type, e.cid_len) == \
            (0, g["sealed_offset"], g["sealed_len"], g["sealed_type"], len(cid))
        assert e.buf.hex() == g["sealed"]
        if not cid:
            assert e.data_len == R.record_len(g["mac"], g["etm"], g["data_len"])
        d = R.decrypt(k, e.buf, e.data_offset, e.data_len, ctr, e.type, ver, cid)
        assert (d.status, d.data_offset, d.data_len, d.type) == (0, g["opened_offset"], g["data_len"], g["type"])
        lo = g["data_offset"]
        assert d.buf[d.data_offset:d.data_offset + d.data_len] == bytes.fromhex(g["plain"])[lo:lo + g["data_len"]]
        seen.add((g["cipher"], g["mac"], g["etm"], bool(cid)))
    assert len(seen) == 24
