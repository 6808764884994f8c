"""X25519 key shares and shared secrets on the GPU, in batches (RFC 7748;
x25519.hip through the C ABI of include/tlsrec.h).

    psa_generate_key + psa_export_public_key (ssl_tls13_generic.c:1566-1582) -> batch_public
    psa_raw_key_agreement (ssl_tls13_keys.c:1457, ssl_tls12_server.c:3028)   -> batch_shared

Every array is a torch uint8 tensor on the device; the calls are asynchronous
on `stream`.  batch_shared writes 32 bytes per connection at any stride, so
its output can be the `shared` field of a tlsrec_tls13_hs_conn array or the
`premaster` field of a tlsrec_tls12_pms_conn array: the key exchange then feeds
keysched.keytab_derive_handshake / tls12.tls12_batch_compute_master on the same
stream with no host step in between.  There is no single-shot form.
"""
from __future__ import annotations

import ctypes

from . import _abi
from .batch import _ptr, _stream
from .keysched import KeyScheduleError, _chk

KEY_BYTES = 32
HS_CONN_BYTES = ctypes.sizeof(_abi.CTls13HsConn)          # 176
HS_SHARED_OFFSET = _abi.CTls13HsConn.shared.offset        # 48
PMS_CONN_BYTES = ctypes.sizeof(_abi.CTls12PmsConn)        # 240
PMS_PREMASTER_OFFSET = _abi.CTls12PmsConn.premaster.offset    # 0

__all__ = ["KEY_BYTES", "KeyScheduleError", "batch_public", "batch_shared", "into_hs_conns", "into_pms_conns"]


def batch_public(priv, pub, count: int, pub_stride: int = KEY_BYTES, stream=None) -> None:
    """pub[pub_stride * i .. + 32) = X25519(priv[32 i ..], 9); priv is count x 32 bytes, packed"""
    _chk("tlsrec_x25519_batch_public", _abi.load().tlsrec_x25519_batch_public(
        _ptr(priv), _ptr(pub), pub_stride, count, _stream(stream)))


def into_hs_conns(conns):
    """(out, out_stride) aiming batch_shared at the `shared` field of a tlsrec_tls13_hs_conn array"""
    return conns.view(-1)[HS_SHARED_OFFSET:], HS_CONN_BYTES


def into_pms_conns(conns):
    """(out, out_stride) aiming batch_shared at the `premaster` field of a tlsrec_tls12_pms_conn array
    (the ECDHE premaster is the raw 32 bytes: pms_len 32)"""
    return conns.view(-1)[PMS_PREMASTER_OFFSET:], PMS_CONN_BYTES


def batch_shared(priv, peer, out, ok, count: int, peer_stride: int = KEY_BYTES, out_stride: int = KEY_BYTES,
                 stream=None) -> None:
    """out[out_stride * i .. + 32) = X25519(priv[32 i ..], peer[peer_stride * i ..]); ok: count x
    uint32, 0 where the output is all zero (the connection is dropped), else 1.  For the fields of
    the next stage's array: out, stride = into_hs_conns(conns), then
    batch_shared(priv, peer, out, ok, count, out_stride=stride)."""
    _chk("tlsrec_x25519_batch_shared", _abi.load().tlsrec_x25519_batch_shared(
        _ptr(priv), _ptr(peer), peer_stride, _ptr(out), out_stride, _ptr(ok), count, _stream(stream)))
