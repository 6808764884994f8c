"""The TLS 1.3 key schedule (RFC 8446 section 7.1) over hashlib / hmac: the
checker of tests/test_tls13_ladder_cpu.py and tests/test_tls13_ladder_gpu.py.
Independent of oracle/keysched.c and of the library: HKDF-Extract and
HKDF-Expand-Label are written out from RFC 5869 and RFC 8446 7.1, the two batch
stages follow the diagram of RFC 8446 7.1, Finished follows 4.4.4 and the PSK
binder 4.2.11.2.

Also a plain FIPS 180-4 compression function (hashlib does not expose one), for
the HMAC midstates the batch kernels take as constants."""
import hashlib
import hmac
import struct

HLEN = {"sha256": 32, "sha384": 48}


def _h(hname):
    return getattr(hashlib, hname)


def extract(hname, salt, ikm):
    """HKDF-Extract (RFC 5869 2.2); salt None or empty = Hash.length zero bytes"""
    return hmac.new(salt or bytes(HLEN[hname]), ikm, _h(hname)).digest()


def hkdf_label(length, label, ctx):
    full = b"tls13 " + label
    return struct.pack(">HB", length, len(full)) + full + bytes([len(ctx)]) + ctx


def expand_label(hname, secret, label, ctx, length):
    """HKDF-Expand-Label (RFC 8446 7.1) = HKDF-Expand (RFC 5869 2.3) with info = HkdfLabel"""
    info, out, t, i = hkdf_label(length, label, ctx), b"", b"", 1
    while len(out) < length:
        t = hmac.new(secret, t + info + bytes([i]), _h(hname)).digest()
        out += t
        i += 1
    return out[:length]


def derive_secret(hname, secret, label, ctx, hashed=True):
    """Derive-Secret(secret, label, messages); `ctx` is Hash(messages) when hashed, else the messages"""
    if not hashed:
        ctx = _h(hname)(ctx).digest()
    return expand_label(hname, secret, label, ctx, HLEN[hname])


def evolve(hname, secret_old, inp):
    """mbedtls_ssl_tls13_evolve_secret: Extract(Derive-Secret(old, "derived", ""), input);
    no old secret = a zero salt, no input = Hash.length zero bytes"""
    salt = derive_secret(hname, secret_old, b"derived", b"", hashed=False) if secret_old else None
    return extract(hname, salt, inp or bytes(HLEN[hname]))


def traffic_keys(hname, secret, key_len, iv_len=12):
    return expand_label(hname, secret, b"key", b"", key_len), expand_label(hname, secret, b"iv", b"", iv_len)


def finished_key(hname, base):
    return expand_label(hname, base, b"finished", b"", HLEN[hname])


def verify_data(hname, fin_key, transcript):
    return hmac.new(fin_key, transcript, _h(hname)).digest()


def calc_finished(hname, base, transcript):
    return verify_data(hname, finished_key(hname, base), transcript)


def psk_binder(hname, psk, resumption, transcript):
    early = evolve(hname, None, psk)
    bk = derive_secret(hname, early, b"res binder" if resumption else b"ext binder", b"", hashed=False)
    return calc_finished(hname, bk, transcript)


def handshake_stage(hname, psk, shared, transcript, key_len):
    """One connection of tlsrec_tls13_keytab_derive_handshake.  Returns a dict:
    c_hs, s_hs, c_fin, s_fin, master, and (key, iv) of both directions."""
    early = evolve(hname, None, psk)
    hs = evolve(hname, early, shared)
    c = derive_secret(hname, hs, b"c hs traffic", transcript)
    s = derive_secret(hname, hs, b"s hs traffic", transcript)
    return {"early": early, "handshake": hs, "c_hs": c, "s_hs": s,
            "c_fin": finished_key(hname, c), "s_fin": finished_key(hname, s),
            "master": evolve(hname, hs, None),
            "c_keys": traffic_keys(hname, c, key_len), "s_keys": traffic_keys(hname, s, key_len)}


def application_stage(hname, master, transcript, key_len):
    """One connection of tlsrec_tls13_keytab_derive_application"""
    c = derive_secret(hname, master, b"c ap traffic", transcript)
    s = derive_secret(hname, master, b"s ap traffic", transcript)
    return {"c_ap": c, "s_ap": s, "exporter": derive_secret(hname, master, b"exp master", transcript),
            "c_keys": traffic_keys(hname, c, key_len), "s_keys": traffic_keys(hname, s, key_len)}


def next_generation(hname, secret):
    """KeyUpdate (RFC 8446 7.2)"""
    return expand_label(hname, secret, b"traffic upd", b"", HLEN[hname])


# ---- FIPS 180-4 compression, for the constant midstates ---------------------
def _primes(n):
    out, k = [], 2
    while len(out) < n:
        if all(k % p for p in out):
            out.append(k)
        k += 1
    return out


def _iroot(n, r):
    lo, hi = 0, 1 << (n.bit_length() // r + 1)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if mid ** r <= n:
            lo = mid
        else:
            hi = mid - 1
    return lo


def _frac_root(p, r, bits):
    """the first `bits` bits of the fractional part of the r-th root of p (FIPS 180-4 4.2.2, 5.3)"""
    return _iroot(p << (r * bits), r) & ((1 << bits) - 1)


_PARAMS = {
    "sha256": (32, 64, (2, 13, 22), (6, 11, 25), (7, 18, 3), (17, 19, 10)),
    "sha384": (64, 80, (28, 34, 39), (14, 18, 41), (1, 8, 7), (19, 61, 6)),
}


def sha2_iv(hname):
    """FIPS 180-4 5.3.3 (SHA-256: square roots of the first 8 primes) and 5.3.4 (SHA-384: of the 9th to 16th)"""
    bits = _PARAMS[hname][0]
    ps = _primes(16)
    return [_frac_root(p, 2, bits) for p in (ps[:8] if hname == "sha256" else ps[8:16])]


def sha2_compress(hname, state, block):
    """one block (64 / 128 bytes) into the 8-word state; returns the new state"""
    bits, rounds, S0, S1, s0, s1 = _PARAMS[hname]
    mask = (1 << bits) - 1
    K = [_frac_root(p, 3, bits) for p in _primes(rounds)]

    def ror(x, n):
        return ((x >> n) | (x << (bits - n))) & mask

    w = [int.from_bytes(block[i * bits // 8:(i + 1) * bits // 8], "big") for i in range(16)]
    for i in range(16, rounds):
        a, b = w[i - 15], w[i - 2]
        w.append((w[i - 16] + (ror(a, s0[0]) ^ ror(a, s0[1]) ^ (a >> s0[2])) + w[i - 7] +
                  (ror(b, s1[0]) ^ ror(b, s1[1]) ^ (b >> s1[2]))) & mask)
    a, b, c, d, e, f, g, h = state
    for i in range(rounds):
        t1 = (h + (ror(e, S1[0]) ^ ror(e, S1[1]) ^ ror(e, S1[2])) + ((e & f) ^ (~e & g & mask)) + K[i] + w[i]) & mask
        t2 = ((ror(a, S0[0]) ^ ror(a, S0[1]) ^ ror(a, S0[2])) + ((a & b) ^ (a & c) ^ (b & c))) & mask
        a, b, c, d, e, f, g, h = (t1 + t2) & mask, a, b, c, (d + t1) & mask, e, f, g
    return [(x + y) & mask for x, y in zip(state, (a, b, c, d, e, f, g, h))]


def hmac_midstates(hname, key):
    """(ipad state, opad state) of HMAC under `key` (at most one block long)"""
    blk = _PARAMS[hname][0] * 2
    k = key + bytes(blk - len(key))
    return (sha2_compress(hname, sha2_iv(hname), bytes(x ^ 0x36 for x in k)),
            sha2_compress(hname, sha2_iv(hname), bytes(x ^ 0x5c for x in k)))


def ladder_constants(hname):
    """What the batch kernels take as constants, as 64-bit integers in the order
    of tlsrec__tls13_ladder_consts: the midstates of the zero salt (8 + 8), the
    midstates of Derive-Secret(Early Secret of an absent PSK, "derived", "")
    (8 + 8), and Hash("") as big-endian words (8 for SHA-256, 6 for SHA-384)."""
    H, wb = HLEN[hname], _PARAMS[hname][0] // 8
    zi, zo = hmac_midstates(hname, bytes(H))
    d0 = derive_secret(hname, evolve(hname, None, None), b"derived", b"", hashed=False)
    di, do = hmac_midstates(hname, d0)
    e = _h(hname)(b"").digest()
    return zi + zo + di + do + [int.from_bytes(e[i:i + wb], "big") for i in range(0, H, wb)]
