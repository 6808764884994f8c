"""The keying-material exporters over hashlib / hmac: the checker of
tests/test_exporter_cpu.py and tests/test_exporter_gpu.py, on the HKDF pieces of
tests/tls13_ref.py and the P_hash of tests/tls12_ref.py.  Independent of
oracle/keysched.c and of the library.  Test-side only.

    TLS 1.3 (RFC 8446 7.5, as mbedtls_ssl_tls13_exporter runs it)  exporter()
    TLS 1.2 (RFC 5705 section 4)                                   export_seed(), export_keying_material()
    the padded first inner message the TLS 1.3 kernel takes        exporter_blocks()
"""
from __future__ import annotations

import hashlib

from tests.tls12_ref import p_hash
from tests.tls13_ref import HLEN, derive_secret, expand_label, hkdf_label

_BLOCK = {"sha256": 64, "sha384": 128}


def _h(hname):
    return getattr(hashlib, hname)


def exporter(hname, secret, label, context, length):
    """Derive-Secret(secret, label, "") then Expand-Label(., "exporter", Hash(context), length)"""
    s1 = derive_secret(hname, secret, label, b"", hashed=False)
    return expand_label(hname, s1, b"exporter", _h(hname)(context).digest(), length)


def exporter_blocks(hname, label):
    """The inner message of the exporter's first HMAC after the ipad block, padded by the
    rules of FIPS 180-4 5.1: HkdfLabel(H, label, Hash("")) || 0x01, 0x80, zeros, and the
    length in bits of ipad block + message.  Returns (big-endian words, block count)."""
    blk = _BLOCK[hname]
    wb, lenb = blk // 16, blk // 8
    msg = hkdf_label(HLEN[hname], label, _h(hname)(b"").digest()) + b"\x01"
    pad = msg + b"\x80" + bytes((-len(msg) - 1 - lenb) % blk) + (8 * (blk + len(msg))).to_bytes(lenb, "big")
    assert len(pad) % blk == 0
    return [int.from_bytes(pad[i:i + wb], "big") for i in range(0, len(pad), wb)], len(pad) // blk


def export_seed(randbytes: bytes, label: bytes, context: bytes | None) -> bytes:
    """label || client_random || server_random [|| uint16(len) || context]; `randbytes` is
    server_random || client_random (after the swap), context None = no context."""
    seed = label + randbytes[32:64] + randbytes[:32]
    if context is not None:
        seed += len(context).to_bytes(2, "big") + context
    return seed


def export_keying_material(hash_name: str, master: bytes, randbytes: bytes, label: bytes, context: bytes | None,
                           n: int) -> bytes:
    return p_hash(hash_name, master, export_seed(randbytes, label, context), n)
