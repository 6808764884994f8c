"""A model of tlsrec_transcript_batch_update in plain Python: the running hash
as its state bytes (chaining words, byte count, hash id, partial block), with
RESET / absorb / SNAPSHOT / HRR and the per-connection error rules of
include/tlsrec.h.  It carries its own FIPS 180-4 compression, so a state can
start from arbitrary chaining words and counts and be compared byte for byte
with what the kernel leaves in device memory; tests/test_transcript_cpu.py
checks it against hashlib."""
import struct

ALG_SHA_256, ALG_SHA_384 = 0x02000009, 0x0200000a
RESET, SNAPSHOT, HRR = 1, 2, 4
BAD_INPUT_DATA = -135
STATE_LEN, SNAPSHOT_LEN = 208, 48

_K512 = [
    0x428a2f98d728ae22, 0x7137449123ef65cd, 0xb5c0fbcfec4d3b2f, 0xe9b5dba58189dbbc, 0x3956c25bf348b538,
    0x59f111f1b605d019, 0x923f82a4af194f9b, 0xab1c5ed5da6d8118, 0xd807aa98a3030242, 0x12835b0145706fbe,
    0x243185be4ee4b28c, 0x550c7dc3d5ffb4e2, 0x72be5d74f27b896f, 0x80deb1fe3b1696b1, 0x9bdc06a725c71235,
    0xc19bf174cf692694, 0xe49b69c19ef14ad2, 0xefbe4786384f25e3, 0x0fc19dc68b8cd5b5, 0x240ca1cc77ac9c65,
    0x2de92c6f592b0275, 0x4a7484aa6ea6e483, 0x5cb0a9dcbd41fbd4, 0x76f988da831153b5, 0x983e5152ee66dfab,
    0xa831c66d2db43210, 0xb00327c898fb213f, 0xbf597fc7beef0ee4, 0xc6e00bf33da88fc2, 0xd5a79147930aa725,
    0x06ca6351e003826f, 0x142929670a0e6e70, 0x27b70a8546d22ffc, 0x2e1b21385c26c926, 0x4d2c6dfc5ac42aed,
    0x53380d139d95b3df, 0x650a73548baf63de, 0x766a0abb3c77b2a8, 0x81c2c92e47edaee6, 0x92722c851482353b,
    0xa2bfe8a14cf10364, 0xa81a664bbc423001, 0xc24b8b70d0f89791, 0xc76c51a30654be30, 0xd192e819d6ef5218,
    0xd69906245565a910, 0xf40e35855771202a, 0x106aa07032bbd1b8, 0x19a4c116b8d2d0c8, 0x1e376c085141ab53,
    0x2748774cdf8eeb99, 0x34b0bcb5e19b48a8, 0x391c0cb3c5c95a63, 0x4ed8aa4ae3418acb, 0x5b9cca4f7763e373,
    0x682e6ff3d6b2b8a3, 0x748f82ee5defb2fc, 0x78a5636f43172f60, 0x84c87814a1f0ab72, 0x8cc702081a6439ec,
    0x90befffa23631e28, 0xa4506cebde82bde9, 0xbef9a3f7b2c67915, 0xc67178f2e372532b, 0xca273eceea26619c,
    0xd186b8c721c0c207, 0xeada7dd6cde0eb1e, 0xf57d4f7fee6ed178, 0x06f067aa72176fba, 0x0a637dc5a2c898a6,
    0x113f9804bef90dae, 0x1b710b35131c471b, 0x28db77f523047d84, 0x32caab7b40c72493, 0x3c9ebe0a15c9bebc,
    0x431d67c49c100d4c, 0x4cc5d4becb3e42b6, 0x597f299cfc657e2a, 0x5fcb6fab3ad6faec, 0x6c44198c4a475817]
# FIPS 180-4 4.2.2: the SHA-256 constants are the high halves of the first 64 SHA-512 ones
_K256 = [k >> 32 for k in _K512[:64]]
_IV256 = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19]
_IV384 = [0xcbbb9d5dc1059ed8, 0x629a292a367cd507, 0x9159015a3070dd17, 0x152fecd8f70e5939,
          0x67332667ffc00b31, 0x8eb44a8768581511, 0xdb0c2e0d64f98fa7, 0x47b5481dbefa4fa4]


class _Shape:
    def __init__(self, alg):
        self.alg = alg
        if alg == ALG_SHA_256:
            self.bits, self.rounds, self.k, self.iv, self.hlen = 32, 64, _K256, _IV256, 32
            self.S0, self.S1, self.s0, self.s1 = (2, 13, 22), (6, 11, 25), (7, 18, 3), (17, 19, 10)
        elif alg == ALG_SHA_384:
            self.bits, self.rounds, self.k, self.iv, self.hlen = 64, 80, _K512, _IV384, 48
            self.S0, self.S1, self.s0, self.s1 = (28, 34, 39), (14, 18, 41), (1, 8, 7), (19, 61, 6)
        else:
            raise ValueError("hash")
        self.block = self.bits * 2          # 64 / 128 bytes
        self.mask = (1 << self.bits) - 1

    def compress(self, h, block):
        """FIPS 180-4 6.2.2 / 6.4.2: the eight chaining words after one block"""
        n, m = self.bits, self.mask

        def ror(x, r):
            return ((x >> r) | (x << (n - r))) & m

        w = [int.from_bytes(block[i * n // 8:(i + 1) * n // 8], "big") for i in range(16)]
        for i in range(16, self.rounds):
            a, b = w[i - 15], w[i - 2]
            w.append((w[i - 16] + (ror(a, self.s0[0]) ^ ror(a, self.s0[1]) ^ (a >> self.s0[2])) + w[i - 7] +
                      (ror(b, self.s1[0]) ^ ror(b, self.s1[1]) ^ (b >> self.s1[2]))) & m)
        a, b, c, d, e, f, g, hh = h
        for i in range(self.rounds):
            t1 = (hh + (ror(e, self.S1[0]) ^ ror(e, self.S1[1]) ^ ror(e, self.S1[2])) + ((e & f) ^ (~e & g & m)) +
                  self.k[i] + w[i]) & m
            t2 = ((ror(a, self.S0[0]) ^ ror(a, self.S0[1]) ^ ror(a, self.S0[2])) + ((a & b) ^ (a & c) ^ (b & c))) & m
            hh, g, f, e, d, c, b, a = g, f, e, (d + t1) & m, c, b, a, (t1 + t2) & m
        return [(x + y) & m for x, y in zip(h, (a, b, c, d, e, f, g, hh))]


class State:
    """one tlsrec_transcript_state"""

    def __init__(self, raw=None):
        raw = bytes(STATE_LEN) if raw is None else bytes(raw)
        assert len(raw) == STATE_LEN
        v = struct.unpack("<8QQII", raw[:80])
        self.h, self.count, self.hash, self.reserved, self.block = list(v[:8]), v[8], v[9], v[10], raw[80:]

    def to_bytes(self):
        return struct.pack("<8QQII", *self.h, self.count, self.hash, self.reserved) + self.block

    def reset(self, alg):
        sh = _Shape(alg)
        self.h, self.count, self.hash, self.reserved, self.block = list(sh.iv), 0, alg, 0, bytes(128)

    def update(self, data):
        sh = _Shape(self.hash)
        fill = self.count % sh.block
        buf = self.block[:fill] + bytes(data)
        self.count = (self.count + len(data)) & (2 ** 64 - 1)
        while len(buf) >= sh.block:
            self.h = sh.compress(self.h, buf[:sh.block])
            buf = buf[sh.block:]
        self.block = buf + bytes(128 - len(buf))

    def digest(self):
        """FIPS 180-4 5.1 padding on a copy; the state goes on"""
        sh = _Shape(self.hash)
        fill = self.count % sh.block
        lenb = sh.bits // 4
        buf = self.block[:fill] + b"\x80"
        buf += bytes(-(len(buf) + lenb) % sh.block) + ((self.count * 8) % (1 << (8 * lenb))).to_bytes(lenb, "big")
        h = list(self.h)
        for i in range(0, len(buf), sh.block):
            h = sh.compress(h, buf[i:i + sh.block])
        return b"".join(x.to_bytes(sh.bits // 8, "big") for x in h)[:sh.hlen]

    def hrr(self):
        """mbedtls_ssl_reset_transcript_for_hrr: a fresh hash over message_hash"""
        d, alg = self.digest(), self.hash
        self.reset(alg)
        self.update(b"\xfe\x00\x00" + bytes([len(d)]) + d)


def batch_update(hash_alg, states, conns, segs, arena, out):
    """states: list of 208-byte states (replaced in place); conns: (state, first_seg, nseg, reserved);
    segs: (off, out_off, len, flags); arena: bytes; out: bytearray.  Returns the status list."""
    assert hash_alg in (ALG_SHA_256, ALG_SHA_384)
    status = []
    for state, first, nseg, reserved in conns:
        bad = state >= len(states) or reserved != 0 or first + nseg > len(segs)
        mine = [] if bad else segs[first:first + nseg]
        for k, (off, out_off, ln, flags) in enumerate(mine):
            bad |= bool(flags & ~(RESET | SNAPSHOT | HRR))
            bad |= off + ln > len(arena)
            bad |= bool(flags & SNAPSHOT) and out_off + SNAPSHOT_LEN > len(out)
            bad |= k == 0 and not flags & RESET and State(states[state]).hash != hash_alg
        if bad:
            status.append(BAD_INPUT_DATA)
            continue
        status.append(0)
        if not mine:
            continue
        st = State(states[state])
        for off, out_off, ln, flags in mine:
            if flags & RESET:
                st.reset(hash_alg)
            st.update(arena[off:off + ln])
            if flags & SNAPSHOT:
                d = st.digest()
                out[out_off:out_off + SNAPSHOT_LEN] = d + bytes(SNAPSHOT_LEN - len(d))
            if flags & HRR:
                st.hrr()
        st.reserved = 0
        states[state] = st.to_bytes()
    return status
