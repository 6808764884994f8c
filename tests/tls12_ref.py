"""Two checkers of the TLS 1.2 PRF for the tests, independent of the code under
test and of each other: P_hash (RFC 5246 section 5) over Python's hmac /
hashlib, and OpenSSL's EVP_KDF "TLS1-PRF" through ctypes.  Test-side only."""
from __future__ import annotations

import ctypes
import ctypes.util
import hashlib
import hmac

HASHES = {"sha256": hashlib.sha256, "sha384": hashlib.sha384}


def p_hash(hash_name: str, secret: bytes, seed: bytes, n: int) -> bytes:
    """PRF(secret, label, random) with seed = label || random."""
    h = HASHES[hash_name]
    a, out = seed, b""
    while len(out) < n:
        a = hmac.new(secret, a, h).digest()
        out += hmac.new(secret, a + seed, h).digest()
    return out[:n]


def split_key_block(keyblk: bytes, key_len: int, iv_len: int):
    """(client_write_key, client_write_iv, server_write_key, server_write_iv), ssl_tls.c:7858-7892"""
    k = key_len
    return (keyblk[:k], keyblk[2 * k:2 * k + iv_len], keyblk[k:2 * k], keyblk[2 * k + iv_len:2 * k + 2 * iv_len])


class _OsslParam(ctypes.Structure):
    """OSSL_PARAM (openssl/core.h)"""
    _fields_ = [("key", ctypes.c_char_p), ("data_type", ctypes.c_uint), ("data", ctypes.c_void_p),
                ("data_size", ctypes.c_size_t), ("return_size", ctypes.c_size_t)]


_UTF8_STRING, _OCTET_STRING = 4, 5           # OSSL_PARAM_UTF8_STRING, OSSL_PARAM_OCTET_STRING
_UNMODIFIED = ctypes.c_size_t(-1).value      # OSSL_PARAM_UNMODIFIED
_crypto = None


def _libcrypto():
    global _crypto
    if _crypto is None:
        L = ctypes.CDLL(ctypes.util.find_library("crypto") or "libcrypto.so.3")
        L.EVP_KDF_fetch.restype = ctypes.c_void_p
        L.EVP_KDF_fetch.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p]
        L.EVP_KDF_CTX_new.restype = ctypes.c_void_p
        L.EVP_KDF_CTX_new.argtypes = [ctypes.c_void_p]
        L.EVP_KDF_derive.restype = ctypes.c_int
        L.EVP_KDF_derive.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        L.EVP_KDF_CTX_free.argtypes = [ctypes.c_void_p]
        L.EVP_KDF_free.argtypes = [ctypes.c_void_p]
        _crypto = L
    return _crypto


def evp_tls1_prf(hash_name: str, secret: bytes, seed: bytes, n: int) -> bytes:
    """The same PRF by OpenSSL 3 (EVP_KDF "TLS1-PRF").  The provider refuses
    an empty secret or an empty seed, so the callers keep those for p_hash."""
    assert secret and seed and n
    L = _libcrypto()
    kdf = L.EVP_KDF_fetch(None, b"TLS1-PRF", None)
    assert kdf, "EVP_KDF_fetch(TLS1-PRF) failed"
    ctx = L.EVP_KDF_CTX_new(kdf)
    assert ctx
    try:
        digest = ctypes.create_string_buffer({"sha256": b"SHA256", "sha384": b"SHA384"}[hash_name])
        sec = ctypes.create_string_buffer(secret, len(secret))
        sd = ctypes.create_string_buffer(seed, len(seed))
        params = (_OsslParam * 4)()
        params[0] = _OsslParam(b"digest", _UTF8_STRING, ctypes.addressof(digest), len(digest.value), _UNMODIFIED)
        params[1] = _OsslParam(b"secret", _OCTET_STRING, ctypes.addressof(sec), len(secret), _UNMODIFIED)
        params[2] = _OsslParam(b"seed", _OCTET_STRING, ctypes.addressof(sd), len(seed), _UNMODIFIED)
        params[3] = _OsslParam(None, 0, None, 0, 0)
        out = ctypes.create_string_buffer(n)
        assert L.EVP_KDF_derive(ctx, out, n, params) == 1, "EVP_KDF_derive(TLS1-PRF) failed"
        return out.raw[:n]
    finally:
        L.EVP_KDF_CTX_free(ctx)
        L.EVP_KDF_free(kdf)
