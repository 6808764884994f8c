"""Checkers for the X25519 batch calls (tests/test_x25519_cpu.py, _gpu.py).

model(k, u): the Montgomery ladder of RFC 7748 section 5 over Python integers,
written from the RFC's pseudocode.  openssl(k, u) / openssl_public(k): the same
through the local libcrypto (ctypes, EVP_PKEY_X25519 = 1034); None where the
library is missing, like tests/_openssl.py.  vectors and the edge set of the
issue live here too, so that the CPU and GPU tests share them.
"""
from __future__ import annotations

import ctypes
import ctypes.util

from tests.prng import prng_bytes

P = 2 ** 255 - 19
A24 = 121665
X = bytes.fromhex


def decode_scalar(k: bytes) -> int:
    e = bytearray(k)
    e[0] &= 248
    e[31] &= 127
    e[31] |= 64
    return int.from_bytes(e, "little")


def decode_u(u: bytes) -> int:
    return (int.from_bytes(u, "little") & ((1 << 255) - 1)) % P


def model(k: bytes, u: bytes) -> bytes:
    """X25519(k, u), 32 bytes (all zero for a small-order u)"""
    kk, x1 = decode_scalar(k), decode_u(u)
    x2, z2, x3, z3, swap = 1, 0, x1, 1, 0
    for t in range(254, -1, -1):
        kt = (kk >> t) & 1
        swap ^= kt
        if swap:
            x2, x3, z2, z3 = x3, x2, z3, z2
        swap = kt
        a = (x2 + z2) % P
        aa = a * a % P
        b = (x2 - z2) % P
        bb = b * b % P
        e = (aa - bb) % P
        c = (x3 + z3) % P
        d = (x3 - z3) % P
        da = d * a % P
        cb = c * b % P
        x3 = (da + cb) ** 2 % P
        z3 = x1 * (da - cb) ** 2 % P
        x2 = aa * bb % P
        z2 = e * (aa + A24 * e) % P
    if swap:
        x2, x3, z2, z3 = x3, x2, z3, z2
    return (x2 * pow(z2, P - 2, P) % P).to_bytes(32, "little")


BASE = (9).to_bytes(32, "little")


def ok_of(out: bytes) -> int:
    return 0 if out == bytes(32) else 1


# ---- libcrypto ----------------------------------------------------------------------
EVP_PKEY_X25519 = 1034
_lib = None


def lib():
    global _lib
    if _lib is None:
        for name in ("libcrypto.so.3", ctypes.util.find_library("crypto")):
            if not name:
                continue
            try:
                _lib = ctypes.CDLL(name)
                break
            except OSError:
                continue
        if _lib is None:
            return None
        L, vp, sz = _lib, ctypes.c_void_p, ctypes.c_size_t
        if not all(hasattr(L, f) for f in ("EVP_PKEY_new_raw_private_key", "EVP_PKEY_new_raw_public_key",
                                           "EVP_PKEY_derive", "EVP_PKEY_get_raw_public_key")):
            _lib = None
            return None
        L.EVP_PKEY_new_raw_private_key.restype = vp
        L.EVP_PKEY_new_raw_private_key.argtypes = [ctypes.c_int, vp, ctypes.c_char_p, sz]
        L.EVP_PKEY_new_raw_public_key.restype = vp
        L.EVP_PKEY_new_raw_public_key.argtypes = [ctypes.c_int, vp, ctypes.c_char_p, sz]
        L.EVP_PKEY_get_raw_public_key.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(sz)]
        L.EVP_PKEY_CTX_new.restype = vp
        L.EVP_PKEY_CTX_new.argtypes = [vp, vp]
        L.EVP_PKEY_derive_init.argtypes = [vp]
        L.EVP_PKEY_derive_set_peer.argtypes = [vp, vp]
        L.EVP_PKEY_derive.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(sz)]
        L.EVP_PKEY_CTX_free.argtypes = [vp]
        L.EVP_PKEY_free.argtypes = [vp]
    return _lib


def openssl_public(k: bytes):
    """X25519(k, 9) by EVP_PKEY_get_raw_public_key; None without libcrypto"""
    L = lib()
    if L is None:
        return None
    key = L.EVP_PKEY_new_raw_private_key(EVP_PKEY_X25519, None, bytes(k), 32)
    assert key
    try:
        out, n = ctypes.create_string_buffer(32), ctypes.c_size_t(32)
        assert L.EVP_PKEY_get_raw_public_key(key, out, ctypes.byref(n)) == 1 and n.value == 32
        return out.raw
    finally:
        L.EVP_PKEY_free(key)


def openssl(k: bytes, u: bytes):
    """X25519(k, u) by EVP_PKEY_derive: 32 bytes, 32 zero bytes where the derive fails
    (libcrypto refuses the all-zero output); None without libcrypto"""
    L = lib()
    if L is None:
        return None
    key = L.EVP_PKEY_new_raw_private_key(EVP_PKEY_X25519, None, bytes(k), 32)
    peer = L.EVP_PKEY_new_raw_public_key(EVP_PKEY_X25519, None, bytes(u), 32)
    assert key and peer
    ctx = L.EVP_PKEY_CTX_new(key, None)
    try:
        assert ctx and L.EVP_PKEY_derive_init(ctx) == 1 and L.EVP_PKEY_derive_set_peer(ctx, peer) == 1
        out, n = ctypes.create_string_buffer(32), ctypes.c_size_t(32)
        if L.EVP_PKEY_derive(ctx, out, ctypes.byref(n)) != 1:
            return bytes(32)
        assert n.value == 32
        return out.raw
    finally:
        L.EVP_PKEY_CTX_free(ctx)
        L.EVP_PKEY_free(peer)
        L.EVP_PKEY_free(key)


# ---- RFC 7748 vectors -----------------------------------------------------------------
RFC_5_2 = [
    (X("a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4"),
     X("e6db6867583030db3594c1a424b15f7c726624ec26b3353b10a903a6d0ab1c4c"),
     X("c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552")),
    (X("4b66e9d4d1b4673c5ad22691957d6af5c11b6421e0ea01d42ca4169e7918ba0d"),
     X("e5210f12786811d3f4b7959d0538ae2c31dbe7106fc03c3efc4cd549c715a493"),
     X("95cbde9476e8907d7aade45cb4b873f88b595a68799fa152e6f8f7647aac7957")),
]
ITER_1 = X("422c8e7a6227d7bca1350b3e2bb7279f7897b87bb6854b783c60e80311ae3079")
ITER_1000 = X("684cf59ba83309552800ef566f2f4d3c1c3887c49360e3875f2eb94d99532c51")
ALICE_PRIV = X("77076d0a7318a57d3c16c17251b26645df4c2f87ebc0992ab177fba51db92c2a")
ALICE_PUB = X("8520f0098930a754748b7ddcb43ef75a0dbf3a0d26381af4eba4a98eaa9b4e6a")
BOB_PRIV = X("5dab087e624a8a4b79e17f8b83800ee66f3bb1292618b6fd1c2f8b27ff88e0eb")
BOB_PUB = X("de9edb7d7b7dc1b4d35b61c2ece435373f8343c85b78674dadfc7e146f882b4f")
SHARED = X("4a5d9d5ba4ce2de1728e3bf480350f25e07e21c947d19e3376f09b3c1e161742")


# ---- the edge set -----------------------------------------------------------------------
def _le(v: int) -> bytes:
    return v.to_bytes(32, "little")


EDGE_SCALARS = [
    bytes(32),
    b"\xff" * 32,
    _le(7 | (1 << 255)),                       # only the bits clamping clears
    _le(1 << 254),                             # only the bit clamping sets
    _le(7 | (1 << 255) | (1 << 254)),
]

# the other small-order points of the well-known low-order list (orders 4 and 8 on the curve and its twist)
LOW_ORDER = [
    X("e0eb7a7c3b41b8ae1656e3faf19fc46ada098deb9c32b1fd866205165f49b800"),
    X("5f9c95bca3508c24b1d0b1559c83ef5b04445cc4581c8e86d8224eddd09f1157"),
]

# the limb boundaries of the kernel's representation: ten limbs of alternately 26 and 25 bits
LIMB_POS = [(51 * i + 1) // 2 for i in range(1, 10)]      # 26, 51, 77, 102, 128, 153, 179, 204, 230


def edge_points():
    base = [0, 1, 2, 9, P - 1, P, P + 1, 2 ** 255 - 1, 2 ** 255 - 20]
    base += [int.from_bytes(b, "little") for b in LOW_ORDER]
    pts = []
    for v in base:
        pts += [_le(v), _le(v | (1 << 255))]
    for p in LIMB_POS:
        pts += [_le(1 << p), _le((1 << p) - 1), _le(1 << (p - 1)), _le(P - (1 << p)), _le(2 ** 255 - (1 << p))]
    return pts


def edge_pairs():
    """(scalar, u): every edge scalar with every edge point, and every edge point under a random scalar"""
    pts = edge_points()
    pairs = [(k, u) for k in EDGE_SCALARS for u in pts]
    pairs += [(prng_bytes(0x25519 + i, 32), u) for i, u in enumerate(pts)]
    pairs += [(k, prng_bytes(0x255190 + i, 32)) for i, k in enumerate(EDGE_SCALARS)]
    return pairs


def random_pairs(seed: int, n: int):
    raw = prng_bytes(seed, 64 * n)
    return [(raw[64 * i:64 * i + 32], raw[64 * i + 32:64 * i + 64]) for i in range(n)]
