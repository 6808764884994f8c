"""AES-CBC + HMAC key slots for TLS 1.2 / DTLS 1.2 batches (include/tlsrec.h,
the tlsrec_keytab_load_cbc section): the MBEDTLS_SSL_MODE_CBC and _CBC_ETM
branches of the reference record path.

A CBC slot lives in the same KeyTable as AEAD slots and is used through the
same batch calls.  Encrypting, the caller places the 16-byte explicit IV at
data_offset - 16 of each record (the engine has no RNG).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _abi
from .batch import KeyTable, _stream

CIPHER_AES_128_CBC = _abi.CIPHER_AES_128_CBC
CIPHER_AES_256_CBC = _abi.CIPHER_AES_256_CBC
MAC_SHA1, MAC_SHA256, MAC_SHA384 = _abi.MAC_SHA1, _abi.MAC_SHA256, _abi.MAC_SHA384
CIPHER_ARIA_128_CBC = _abi.CIPHER_ARIA_128_CBC
CIPHER_ARIA_256_CBC = _abi.CIPHER_ARIA_256_CBC
CIPHER_CAMELLIA_128_CBC = _abi.CIPHER_CAMELLIA_128_CBC
CIPHER_CAMELLIA_256_CBC = _abi.CIPHER_CAMELLIA_256_CBC
CBC_KEYLEN = {CIPHER_AES_128_CBC: 16, CIPHER_AES_256_CBC: 32}           # AES: every MAC
# ARIA / Camellia: one MAC each, as every suite of the reference pairs them
CBC_ALT_KEYLEN = {CIPHER_ARIA_128_CBC: 16, CIPHER_ARIA_256_CBC: 32,
                  CIPHER_CAMELLIA_128_CBC: 16, CIPHER_CAMELLIA_256_CBC: 32}
CBC_ALL_KEYLEN = {**CBC_KEYLEN, **CBC_ALT_KEYLEN}                       # every id tlsrec_keytab_load_cbc takes
CBC_ALT_MAC = {CIPHER_ARIA_128_CBC: MAC_SHA256, CIPHER_ARIA_256_CBC: MAC_SHA384,
               CIPHER_CAMELLIA_128_CBC: MAC_SHA256, CIPHER_CAMELLIA_256_CBC: MAC_SHA384}
MACLEN = {MAC_SHA1: 20, MAC_SHA256: 32, MAC_SHA384: 48}
IVLEN = 16
CBC_KEY_MATERIAL = _abi.CBC_KEY_MATERIAL


def key_material(cipher: int, mac: int, etm: int, key: bytes, mac_key: bytes, tls_minor: int = 3) -> np.ndarray:
    """One tlsrec_cbc_key_material record (numpy structured array of 1)."""
    km = np.zeros(1, dtype=CBC_KEY_MATERIAL)
    km["cipher"] = cipher
    km["tls_minor"] = tls_minor
    km["mac"] = mac
    km["etm"] = etm
    km["key"][0, :len(key)] = np.frombuffer(bytes(key), dtype=np.uint8)
    km["mac_key"][0, :len(mac_key)] = np.frombuffer(bytes(mac_key), dtype=np.uint8)
    return km


def load_status(kt: KeyTable, keys, first: int = 0, stream=None) -> int:
    """tlsrec_keytab_load_cbc, returning its status.  keys: numpy array of
    CBC_KEY_MATERIAL (host) or a uint8 device tensor of count * 128 bytes."""
    if isinstance(keys, np.ndarray):
        keys = np.ascontiguousarray(keys, dtype=CBC_KEY_MATERIAL)
        count, on_dev, p = len(keys), 0, keys.ctypes.data
    else:
        count, on_dev, p = keys.numel() // 128, 1, keys.data_ptr()
    return _abi.load().tlsrec_keytab_load_cbc(kt.handle, first, count, p, on_dev, _stream(stream))


def load(kt: KeyTable, keys, first: int = 0, stream=None) -> None:
    r = load_status(kt, keys, first, stream)
    if r != 0:
        raise RuntimeError(f"tlsrec_keytab_load_cbc failed: {r:#x}")


def record_len(mac: int, etm: int, content_len: int) -> int:
    """explicit IV + ciphertext (+ MAC) bytes of a record of content_len bytes"""
    return _abi.load().tlsrec_cbc_record_len(mac, etm, content_len)


def minlen(mac: int, etm: int) -> int:
    return _abi.load().tlsrec_cbc_minlen(mac, etm)


def _split_out(ks: np.ndarray):
    return ks[0:1].copy(), ks[1:2].copy()


def split_key_block(cipher: int, mac: int, keyblk: bytes):
    """(status, client_write, server_write): the CBC layout of the TLS 1.2 key block"""
    ks = np.zeros(2, dtype=CBC_KEY_MATERIAL)
    buf = (ctypes.c_ubyte * max(1, len(keyblk))).from_buffer_copy(bytes(keyblk) or b"\0")
    r = _abi.load().tlsrec_tls12_split_key_block_cbc(cipher, mac, ctypes.addressof(buf), len(keyblk), ks.ctypes.data)
    return (r,) + _split_out(ks)


def make_keys(prf: int, cipher: int, mac: int, master: bytes, randbytes: bytes):
    """(status, client_write, server_write): PRF(master, "key expansion", randbytes) + the split"""
    assert len(master) == 48 and len(randbytes) == 64
    ks = np.zeros(2, dtype=CBC_KEY_MATERIAL)
    m = (ctypes.c_ubyte * 48).from_buffer_copy(bytes(master))
    rb = (ctypes.c_ubyte * 64).from_buffer_copy(bytes(randbytes))
    r = _abi.load().tlsrec_tls12_make_keys_cbc(prf, cipher, mac, ctypes.addressof(m), ctypes.addressof(rb),
                                               ks.ctypes.data)
    return (r,) + _split_out(ks)
