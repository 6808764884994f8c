"""Python mirror of the reference record-protection interface.

    Transform  ~ struct mbedtls_ssl_transform, populated like
                 mbedtls_ssl_tls13_populate_transform (ssl_tls13_keys.c:922)
                 / the AEAD branch of ssl_tls12_populate_transform
                 (ssl_tls.c:7768-7797); Transform.cbc: its CBC + HMAC
                 branch (ssl_tls.c:7798-7847)
    Record     ~ mbedtls_record (ssl_misc.h:1163-1188), incl. the DTLS 1.2
                 connection ID (cid)
    encrypt_buf(transform, rec)  ~ mbedtls_ssl_encrypt_buf (ssl_msg.c:784)
    decrypt_buf(transform, rec)  ~ mbedtls_ssl_decrypt_buf (ssl_msg.c:1270)

Same argument meaning, same in-place behaviour, same error codes
(``mbedtls_amd.ERR_SSL_*``).  All record bytes are processed by the HIP
kernels in libtlsrec.so.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

from . import _abi


@dataclass
class Record:
    ctr: bytes
    type: int
    ver: bytes
    buf: bytearray
    data_offset: int
    data_len: int
    buf_len: int = field(default=-1)
    cid: bytes = b""            # rec->cid / cid_len (DTLS 1.2 connection ID)

    def __post_init__(self):
        if self.buf_len < 0:
            self.buf_len = len(self.buf)

    def data(self) -> bytes:
        return bytes(self.buf[self.data_offset:self.data_offset + self.data_len])


class Transform:
    """One connection's record-protection state (both directions)."""

    def __init__(self, tls_version: int, cipher: int, key_enc: bytes, key_dec: bytes,
                 iv_enc: bytes, iv_dec: bytes, granularity: int = 16):
        self._lib = _abi.load()
        self._t = _abi.CTransform()
        r = self._lib.tlsrec_transform_setup_ex(ctypes.byref(self._t), tls_version, cipher,
                                                bytes(key_enc), bytes(key_dec), bytes(iv_enc),
                                                bytes(iv_dec), granularity)
        if r != 0:
            raise RuntimeError(f"tlsrec_transform_setup failed: {r:#x}")
        self.tls_version, self.cipher = tls_version, cipher

    @classmethod
    def cbc(cls, tls_version: int, cipher: int, mac: int, etm: int, key_enc: bytes, key_dec: bytes,
            mac_enc: bytes, mac_dec: bytes) -> "Transform":
        """A CBC + HMAC transform (tlsrec_transform_setup_cbc): cipher a CIPHER_*_CBC id, mac a
        MAC_*, etm 0 = MAC-then-encrypt / 1 = encrypt-then-MAC.  encrypt_buf draws the explicit
        IV itself and writes it in front of the content."""
        self = cls.__new__(cls)
        self._lib = _abi.load()
        self._t = _abi.CTransform()
        r = self._lib.tlsrec_transform_setup_cbc(ctypes.byref(self._t), tls_version, cipher, mac, etm,
                                                 bytes(key_enc), bytes(key_dec), bytes(mac_enc), bytes(mac_dec))
        if r != 0:
            self._t = None
            raise RuntimeError(f"tlsrec_transform_setup_cbc failed: {r:#x}")
        self.tls_version, self.cipher = tls_version, cipher
        return self

    def set_cid(self, in_cid: bytes, out_cid: bytes) -> None:
        """transform->in_cid / out_cid (DTLS 1.2 connection IDs)."""
        r = self._lib.tlsrec_transform_set_cid(ctypes.byref(self._t), bytes(in_cid), len(in_cid),
                                               bytes(out_cid), len(out_cid))
        if r != 0:
            raise RuntimeError(f"tlsrec_transform_set_cid failed: {r:#x}")

    @property
    def slots(self):
        return self._t.slot_enc, self._t.slot_dec

    @property
    def fixed_ivlen(self):
        return self._t.fixed_ivlen

    def close(self):
        if self._t is not None:
            self._lib.tlsrec_transform_free(ctypes.byref(self._t))
            self._t = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, fn, rec: Record) -> int:
        c = _abi.CRecord()
        c.ctr[:] = list(rec.ctr)
        c.type = rec.type
        c.ver[:] = list(rec.ver)
        n = max(1, len(rec.buf))
        if len(rec.buf) == 0:
            rec.buf.extend(b"\0")
        cbuf = (ctypes.c_ubyte * n).from_buffer(rec.buf)
        c.buf = ctypes.addressof(cbuf)
        c.buf_len = rec.buf_len
        c.data_offset = rec.data_offset
        c.data_len = rec.data_len
        c.cid_len = len(rec.cid)
        c.cid[:len(rec.cid)] = list(rec.cid)
        r = fn(None, ctypes.byref(self._t), ctypes.byref(c))
        del cbuf
        rec.type, rec.ver = c.type, bytes(c.ver)
        rec.data_offset, rec.data_len = c.data_offset, c.data_len
        rec.cid = bytes(c.cid[:c.cid_len])
        return r

    def encrypt_buf(self, rec: Record) -> int:
        return self._call(self._lib.tlsrec_encrypt_buf, rec)

    def decrypt_buf(self, rec: Record) -> int:
        return self._call(self._lib.tlsrec_decrypt_buf, rec)


def encrypt_buf(transform: Transform, rec: Record) -> int:
    return transform.encrypt_buf(rec)


def decrypt_buf(transform: Transform, rec: Record) -> int:
    return transform.decrypt_buf(rec)
