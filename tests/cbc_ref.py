"""Reference model of the AES-CBC + HMAC record path for the tests: the
MBEDTLS_SSL_MODE_CBC / _CBC_ETM branches of mbedtls_ssl_encrypt_buf
(library/ssl_msg.c:906-968, :1080-1253) and mbedtls_ssl_decrypt_buf
(:1435-1702, :1717-1801) restated in plain Python, independent of the code
under test: HMAC from hashlib / hmac, AES-CBC without padding from OpenSSL's
libcrypto through ctypes.  Test-side only.

A transform direction is a `Key`; a record is (buf, data_offset, data_len, ctr,
type, ver[, cid]).  encrypt() / decrypt() return a `Result` with the status,
data_offset, data_len, type, cid_len and buffer bytes the reference leaves.
On encrypt the explicit IV is read from buf[data_offset - 16 : data_offset]
(the engine's one divergence: the reference draws it at random).  On a
non-zero status the bytes are returned as given: they are unspecified.
"""
from __future__ import annotations

import ctypes
import ctypes.util
import hashlib
import hmac
from dataclasses import dataclass

CIPHER_AES_128_CBC, CIPHER_AES_256_CBC = 23, 24
MAC_SHA1, MAC_SHA256, MAC_SHA384 = 1, 2, 3
KEYLEN = {CIPHER_AES_128_CBC: 16, CIPHER_AES_256_CBC: 32}
HASH = {MAC_SHA1: hashlib.sha1, MAC_SHA256: hashlib.sha256, MAC_SHA384: hashlib.sha384}
MACLEN = {MAC_SHA1: 20, MAC_SHA256: 32, MAC_SHA384: 48}
IVLEN = 16

E_BAD_INPUT_DATA = -135
E_BUFFER_TOO_SMALL = -138
E_INVALID_MAC = -0x7180
E_INVALID_RECORD = -0x7200
E_INTERNAL_ERROR = -0x6C00
E_UNEXPECTED_CID = -0x6000
MSG_CID = 25
OUT_CONTENT_LEN = 16384
GRANULARITY = 16

_crypto = None


def _lib():
    global _crypto
    if _crypto is None:
        L = ctypes.CDLL(ctypes.util.find_library("crypto") or "libcrypto.so.3")
        L.EVP_CIPHER_CTX_new.restype = ctypes.c_void_p
        L.EVP_CIPHER_CTX_free.argtypes = [ctypes.c_void_p]
        L.EVP_aes_128_cbc.restype = ctypes.c_void_p
        L.EVP_aes_256_cbc.restype = ctypes.c_void_p
        L.EVP_CipherInit_ex.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p,
                                        ctypes.c_char_p, ctypes.c_int]
        L.EVP_CIPHER_CTX_set_padding.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.EVP_CipherUpdate.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int),
                                       ctypes.c_char_p, ctypes.c_int]
        _crypto = L
    return _crypto


def aes_cbc(key: bytes, iv: bytes, data: bytes, encrypt: bool) -> bytes:
    """AES-CBC over whole blocks, no padding"""
    assert len(data) % 16 == 0 and len(iv) == 16 and len(key) in (16, 32)
    if not data:
        return b""
    L = _lib()
    ctx = L.EVP_CIPHER_CTX_new()
    try:
        c = L.EVP_aes_128_cbc() if len(key) == 16 else L.EVP_aes_256_cbc()
        assert L.EVP_CipherInit_ex(ctx, c, None, key, iv, 1 if encrypt else 0) == 1
        L.EVP_CIPHER_CTX_set_padding(ctx, 0)
        out = ctypes.create_string_buffer(len(data) + 32)
        n = ctypes.c_int()
        assert L.EVP_CipherUpdate(ctx, out, ctypes.byref(n), data, len(data)) == 1
        assert n.value == len(data)
        return out.raw[:n.value]
    finally:
        L.EVP_CIPHER_CTX_free(ctx)


@dataclass
class Key:
    cipher: int
    mac: int
    etm: int
    key: bytes
    mac_key: bytes
    cid: bytes = b""           # out_cid when encrypting, in_cid when decrypting


@dataclass
class Result:
    status: int
    data_offset: int
    data_len: int
    type: int
    cid_len: int
    buf: bytes


def add_data(ctr: bytes, rtype: int, ver: bytes, length: int, cid: bytes = b"") -> bytes:
    """ssl_extract_add_data_from_record for TLS 1.2 (ssl_msg.c:568-735)"""
    if cid:
        return (b"\xff" * 8 + bytes([MSG_CID, len(cid), MSG_CID]) + bytes(ver) + bytes(ctr) + bytes(cid) +
                length.to_bytes(2, "big"))
    return bytes(ctr) + bytes([rtype]) + bytes(ver) + length.to_bytes(2, "big")


def _mac(k: Key, ctr, rtype, ver, data: bytes, cid: bytes) -> bytes:
    return hmac.new(k.mac_key, add_data(ctr, rtype, ver, len(data), cid) + data, HASH[k.mac]).digest()


def encrypt(k: Key, buf: bytes, data_offset: int, data_len: int, ctr: bytes, rtype: int, ver: bytes) -> Result:
    buf = bytearray(buf)
    maclen = MACLEN[k.mac]
    cid_len = 0

    def res(status):
        return Result(status, data_offset, data_len, rtype, cid_len, bytes(buf))

    if len(buf) < data_offset or len(buf) - data_offset < data_len:            # :814-823
        return res(E_INTERNAL_ERROR)
    if data_len > OUT_CONTENT_LEN:                                             # :833-839
        return res(E_BAD_INPUT_DATA)
    post_avail = len(buf) - (data_len + data_offset)
    cid_len = len(k.cid)                                                       # :874
    if k.cid:                                                                  # :878-898
        pad = (-(data_len + 1)) % GRANULARITY
        if post_avail == 0:
            return res(E_BUFFER_TOO_SMALL)
        buf[data_offset + data_len] = rtype
        if post_avail - 1 < pad:
            return res(E_BUFFER_TOO_SMALL)
        buf[data_offset + data_len + 1:data_offset + data_len + 1 + pad] = bytes(pad)
        data_len += 1 + pad
        rtype = MSG_CID
    post_avail = len(buf) - (data_len + data_offset)
    auth_done = 0
    if not k.etm:                                                              # :906-968
        if post_avail < maclen:
            return res(E_BUFFER_TOO_SMALL)
        mac = _mac(k, ctr, rtype, ver, bytes(buf[data_offset:data_offset + data_len]), k.cid)
        buf[data_offset + data_len:data_offset + data_len + maclen] = mac
        data_len += maclen
        post_avail -= maclen
        auth_done += 1
    padlen = IVLEN - (data_len + 1) % IVLEN                                    # :1092-1095
    if padlen == IVLEN:
        padlen = 0
    if post_avail < padlen + 1:                                                # :1098
        return res(E_BUFFER_TOO_SMALL)
    buf[data_offset + data_len:data_offset + data_len + padlen + 1] = bytes([padlen]) * (padlen + 1)
    data_len += padlen + 1
    post_avail -= padlen + 1
    if data_offset < IVLEN:                                                    # :1116
        return res(E_BUFFER_TOO_SMALL)
    iv = bytes(buf[data_offset - IVLEN:data_offset])                           # the caller's IV (:1124 draws it)
    buf[data_offset:data_offset + data_len] = aes_cbc(k.key, iv, bytes(buf[data_offset:data_offset + data_len]), True)
    data_offset -= IVLEN                                                       # :1186-1188
    data_len += IVLEN
    if auth_done == 0:                                                         # :1191-1250
        if post_avail < maclen:
            return res(E_BUFFER_TOO_SMALL)
        mac = _mac(k, ctr, rtype, ver, bytes(buf[data_offset:data_offset + data_len]), k.cid)
        buf[data_offset + data_len:data_offset + data_len + maclen] = mac
        data_len += maclen
    return res(0)


def decrypt(k: Key, buf: bytes, data_offset: int, data_len: int, ctr: bytes, rtype: int, ver: bytes,
            cid: bytes = b"") -> Result:
    buf = bytearray(buf)
    maclen = MACLEN[k.mac]

    def res(status):
        return Result(status, data_offset, data_len, rtype, 0, bytes(buf))

    if len(buf) < data_offset or len(buf) - data_offset < data_len:            # :1302-1308
        return res(E_INTERNAL_ERROR)
    if bytes(cid) != bytes(k.cid):                                             # :1317-1320
        return res(E_UNEXPECTED_CID)
    if data_len < 2 * IVLEN or data_len < IVLEN + maclen + 1:                  # :1472-1482
        return res(E_INVALID_MAC)
    auth_done = 0
    if k.etm:                                                                  # :1488-1547
        data_len -= maclen
        want = _mac(k, ctr, rtype, ver, bytes(buf[data_offset:data_offset + data_len]), cid)
        if not hmac.compare_digest(want, bytes(buf[data_offset + data_len:data_offset + data_len + maclen])):
            return res(E_INVALID_MAC)
        auth_done += 1
    if data_len % IVLEN != 0:                                                  # :1557-1562
        return res(E_INVALID_MAC)
    iv = bytes(buf[data_offset:data_offset + IVLEN])                           # :1569-1573
    data_offset += IVLEN
    data_len -= IVLEN
    buf[data_offset:data_offset + data_len] = aes_cbc(k.key, iv, bytes(buf[data_offset:data_offset + data_len]), False)
    data = buf[data_offset:data_offset + data_len]
    padlen = data[-1]                                                          # :1627
    if auth_done == 1:
        correct = data_len >= padlen + 1
    else:
        correct = data_len >= maclen + padlen + 1
    if not correct:
        padlen = 0
    padlen += 1
    padding_idx = data_len - padlen                                            # :1665-1692
    num_checks = min(256, data_len)
    pad_count = sum(1 for idx in range(data_len - num_checks, data_len)
                    if idx >= padding_idx and data[idx] == padlen - 1)
    correct = correct and pad_count == padlen
    if not correct:
        padlen = 0
    data_len -= padlen                                                         # :1700
    if auth_done == 0:                                                         # :1718-1793
        data_len -= maclen
        want = _mac(k, ctr, rtype, ver, bytes(data[:data_len]), cid)
        if not hmac.compare_digest(want, bytes(data[data_len:data_len + maclen])):
            correct = False
    if not correct:
        return res(E_INVALID_MAC)
    if cid:                                                                    # :1822-1828
        n = data_len
        while n > 0 and data[n - 1] == 0:
            n -= 1
        if n == 0:
            return res(E_INVALID_RECORD)
        rtype = data[n - 1]
        data_len = n - 1
    return res(0)


def record_len(mac: int, etm: int, content_len: int) -> int:
    """explicit IV + ciphertext (+ MAC) of a record without a CID"""
    body = content_len + (0 if etm else MACLEN[mac])
    padlen = IVLEN - (body + 1) % IVLEN
    if padlen == IVLEN:
        padlen = 0
    return IVLEN + body + padlen + 1 + (MACLEN[mac] if etm else 0)


def minlen(mac: int, etm: int) -> int:
    """ssl_tls.c:7822-7835"""
    ml = MACLEN[mac]
    return (ml + IVLEN if etm else ml + IVLEN - ml % IVLEN) + IVLEN
