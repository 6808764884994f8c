"""Checker of the TLS 1.2 handshake derivations for the tests (ssl_compute_master,
ssl_tls.c:6251-6452; the random swap, :6479-6488; ssl_calc_finished_tls_generic,
:7209-7261; the RFC 4279 premaster of the PSK exchanges, :6307-6366), built on the
P_hash of tests/tls12_ref.py and cross-checked by OpenSSL's EVP_KDF "TLS1-PRF"
wherever secret and seed are non-empty.  Independent of the code under test."""
from __future__ import annotations

from tests.tls12_ref import evp_tls1_prf, p_hash

HLEN = {"sha256": 32, "sha384": 48}
PMS_CONN = 240          # premaster[128] || client_random[32] || server_random[32] || session_hash[48]
CONN = 112              # master[48] || server_random[32] || client_random[32]
FINISHED_LABEL = {0: b"client finished", 1: b"server finished"}     # by MBEDTLS_SSL_IS_CLIENT / _IS_SERVER


def prf(hname: str, secret: bytes, seed: bytes, n: int) -> bytes:
    want = p_hash(hname, secret, seed, n)
    if secret and seed and n:
        try:
            other = evp_tls1_prf(hname, secret, seed, n)
        except (OSError, AttributeError):       # no OpenSSL 3 on this machine: hashlib alone
            other = want
        assert other == want
    return want


def master(hname: str, premaster: bytes, randbytes: bytes, session_hash: bytes | None = None) -> bytes:
    """randbytes: client_random || server_random; session_hash given = extended master secret (RFC 7627)"""
    if session_hash is not None:
        assert len(session_hash) == HLEN[hname]
        return prf(hname, premaster, b"extended master secret" + session_hash, 48)
    assert len(randbytes) == 64
    return prf(hname, premaster, b"master secret" + randbytes, 48)


def swap(randbytes: bytes) -> bytes:
    """client_random || server_random -> server_random || client_random"""
    assert len(randbytes) == 64
    return randbytes[32:] + randbytes[:32]


def conn_out(hname: str, pms_conn: bytes, pms_len: int, extended_ms: bool) -> bytes:
    """the tlsrec_tls12_conn a tlsrec_tls12_pms_conn becomes"""
    assert len(pms_conn) == PMS_CONN and 1 <= pms_len <= 128
    rb = pms_conn[128:192]
    sh = pms_conn[192:192 + HLEN[hname]] if extended_ms else None
    return master(hname, pms_conn[:pms_len], rb, sh) + swap(rb)


def verify_data(hname: str, master_secret: bytes, transcript_hash: bytes, from_: int) -> bytes:
    assert len(master_secret) == 48 and len(transcript_hash) == HLEN[hname]
    return prf(hname, master_secret, FINISHED_LABEL[from_] + transcript_hash, 12)


def psk_premaster(psk: bytes, other: bytes | None = None) -> bytes:
    """uint16 len || other || uint16 len || psk; plain PSK: other = len(psk) zero bytes (RFC 4279 section 2)"""
    if other is None:
        other = bytes(len(psk))
    return len(other).to_bytes(2, "big") + other + len(psk).to_bytes(2, "big") + psk
