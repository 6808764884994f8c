"""Reference model of the ARIA-CBC / Camellia-CBC + HMAC record path: the
record logic is tests/cbc_ref.py's encrypt() / decrypt() themselves (which 24
golden AES records pin), run with that module's block function swapped for the
duration of a call.  The swapped-in function is OpenSSL's EVP_aria_*_cbc /
EVP_camellia_*_cbc through ctypes, no padding: independent of the code under
test.  An AES key passes straight through.  Test-side only."""
from __future__ import annotations

import ctypes
from contextlib import contextmanager

from tests import cbc_ref as R

CIPHER_ARIA_128_CBC, CIPHER_ARIA_256_CBC, CIPHER_CAMELLIA_128_CBC, CIPHER_CAMELLIA_256_CBC = 26, 27, 28, 29
KEYLEN = {CIPHER_ARIA_128_CBC: 16, CIPHER_ARIA_256_CBC: 32, CIPHER_CAMELLIA_128_CBC: 16, CIPHER_CAMELLIA_256_CBC: 32}
# the one MAC each id is negotiated with (library/ssl_ciphersuites.c)
MAC_OF = {CIPHER_ARIA_128_CBC: R.MAC_SHA256, CIPHER_ARIA_256_CBC: R.MAC_SHA384,
          CIPHER_CAMELLIA_128_CBC: R.MAC_SHA256, CIPHER_CAMELLIA_256_CBC: R.MAC_SHA384}
SUITES = sorted(MAC_OF.items())
_EVP = {CIPHER_ARIA_128_CBC: "EVP_aria_128_cbc", CIPHER_ARIA_256_CBC: "EVP_aria_256_cbc",
        CIPHER_CAMELLIA_128_CBC: "EVP_camellia_128_cbc", CIPHER_CAMELLIA_256_CBC: "EVP_camellia_256_cbc"}
ALL_KEYLEN = {**R.KEYLEN, **KEYLEN}

Key, Result = R.Key, R.Result
_encrypt, _decrypt, _aes_cbc = R.encrypt, R.decrypt, R.aes_cbc


def evp_cbc(cipher: int, key: bytes, iv: bytes, data: bytes, encrypt: bool) -> bytes:
    """CBC over whole blocks, no padding, under EVP's cipher for `cipher`"""
    assert len(data) % 16 == 0 and len(iv) == 16 and len(key) == KEYLEN[cipher]
    if not data:
        return b""
    L = R._lib()
    f = getattr(L, _EVP[cipher])
    f.restype = ctypes.c_void_p
    ctx = L.EVP_CIPHER_CTX_new()
    try:
        assert L.EVP_CipherInit_ex(ctx, f(), None, key, iv, 1 if encrypt else 0) == 1
        L.EVP_CIPHER_CTX_set_padding(ctx, 0)
        out = ctypes.create_string_buffer(len(data) + 32)
        n = ctypes.c_int()
        assert L.EVP_CipherUpdate(ctx, out, ctypes.byref(n), data, len(data)) == 1
        assert n.value == len(data)
        return out.raw[:n.value]
    finally:
        L.EVP_CIPHER_CTX_free(ctx)


def block_cbc(cipher: int, key: bytes, iv: bytes, data: bytes, encrypt: bool) -> bytes:
    return evp_cbc(cipher, key, iv, data, encrypt) if cipher in _EVP else _aes_cbc(key, iv, data, encrypt)


@contextmanager
def _block_function(cipher: int):
    if cipher not in _EVP:
        yield
        return
    R.aes_cbc = lambda key, iv, data, enc: evp_cbc(cipher, key, iv, data, enc)
    try:
        yield
    finally:
        R.aes_cbc = _aes_cbc


def encrypt(k, *args, **kw):
    with _block_function(k.cipher):
        return _encrypt(k, *args, **kw)


def decrypt(k, *args, **kw):
    with _block_function(k.cipher):
        return _decrypt(k, *args, **kw)


@contextmanager
def as_model():
    """cbc_ref.encrypt / decrypt are this module's while the block runs, for
    helpers that call them by name (cbclib, cbc_frames_ref)"""
    R.encrypt, R.decrypt = encrypt, decrypt
    try:
        yield
    finally:
        R.encrypt, R.decrypt = _encrypt, _decrypt
