"""Skewed key runs, edge lengths and exceptional records for the AES-GCM wave
passes (launch code -8) and paired wave passes (-32) of tlsrec_gcm_kernel.
Test side only, vectorised numpy: a batch here holds up to a few hundred
thousand records, which tests/batchlib.py's record-at-a-time Batch is too slow
for.

* case_table(cu): the nine (L, code) families, each sized from the device's CU
  count so that tlsrec_plan.h gcm_plan() picks the family and a wave runs
  several rounds (rpw >= min(3 R, 64), R = 64 / L records per round);
* skewed_keyidx(): per-record slot numbers whose per-key counts follow a fixed
  pattern -- keys without a record, keys with one, runs of R - 1 / R / R + 1
  records, runs longer than a pair's chunk and than a workgroup -- behind a
  fixed permutation, so the bucket pass does the ordering;
* edge_lengths(): lengths at the block counts m near the multiples of L, on
  which the lane-power GHASH layout depends (d = (m - q) mod L);
* RunBatch: the arena, descriptors and keys of one case, the EVP checks of
  tests/test_evp_parity_gpu.py over any subset of it, and the exceptional
  records of tests/test_gcm_runs_gpu.py (b) with their expectation from the
  oracle, one record at a time.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import mbedtls_amd as M
import oracle as O
from mbedtls_amd import _abi

EDGE = np.array([0, 1, 15, 16, 17, 1400, 16383], dtype=np.uint32)
NR = {M.CIPHER_AES_128_GCM: 10, M.CIPHER_AES_256_GCM: 14}
SUITES = [(M.CIPHER_AES_128_GCM, M.VERSION_TLS1_2), (M.CIPHER_AES_256_GCM, M.VERSION_TLS1_3)]
SUITE_IDS = ["aes128-tls12", "aes256-tls13"]
SPARE_SLOTS = 8                   # slots of a case's key table that never hold a key


def threads():
    import bench
    return bench.host_cores()[0]


def layout(n, head, rng, span=None, misalign=False):
    """lengths (25 % edge values, 75 % uniform 0..2048, every edge value at
    least 100 times; or uniform in span), 128-B aligned record buffers with
    tag / padding room (misalign: each buffer starts 0..127 bytes into its
    128-B slot)"""
    if span:
        lens = rng.integers(span[0], span[1] + 1, n).astype(np.uint32)
    else:
        lens = rng.integers(0, 2049, n).astype(np.uint32)
        pick = rng.random(n) < 0.25
        lens[pick] = EDGE[rng.integers(0, len(EDGE), int(pick.sum()))]
        lens[:len(EDGE) * 100] = np.tile(EDGE, 100)
    size = head + lens.astype(np.uint64) + 48
    al = (size + 127) // 128 * 128 + (128 if misalign else 0)
    off = np.zeros(n, dtype=np.uint64)
    off[1:] = np.cumsum(al)[:-1]
    if misalign:
        off += rng.integers(0, 128, n).astype(np.uint64)
    return lens, size, off, int(off[-1] + al[-1])


def keys(cipher, nkeys, rng):
    kl = M.KEYLEN[cipher]
    k = rng.integers(0, 256, (nkeys, 32), dtype=np.uint8)
    k[:, kl:] = 0
    ivs = rng.integers(0, 256, (nkeys, 12), dtype=np.uint8)
    return k, ivs


# ---- the cases ------------------------------------------------------------------
def default_knobs(**over):
    """tlsrec::GcmKnobs of an empty environment, with a case's switches"""
    k = dict(waves=16, wp=-1, g5=1, treemul=-1, hbuild=1, pair=1, grouped=1, srecs=0, pair_l=0,
             pair_small_min=12, pair_small_max=256, pair_big_max=40, lanes=0)
    k.update(over)
    return _abi.GcmKnobs(**k)


# every TLSREC_* switch gcm_plan() or batch() reads: a test clears them all, then sets its case's
SWITCHES = ("TLSREC_GCM_WP", "TLSREC_GCM_G5", "TLSREC_GCM_TREEMUL", "TLSREC_GCM_HBUILD", "TLSREC_GCM_PAIR",
            "TLSREC_GROUPED", "TLSREC_GCM_SRECS", "TLSREC_GCM_PAIR_L", "TLSREC_GCM_PAIR_SMALL_MIN",
            "TLSREC_GCM_PAIR_SMALL_MAX", "TLSREC_GCM_PAIR_BIG_MAX", "TLSREC_GCM_LANES", "TLSREC_STREAM_SRC")

# id: (L, launch code, waves per workgroup, size hint, environment, knobs, lanes argument,
#      band of n // nloaded that selects the family (None: the switches alone do), mean records per key used)
_FAMILIES = {
    "pair-2": (2, -32, 16, 100, {"TLSREC_GCM_PAIR_L": "2"}, {"pair_l": 2}, 0, (12, 256), 20),
    "pair-4": (4, -32, 16, 100, {"TLSREC_GCM_PAIR_L": "4"}, {"pair_l": 4}, 0, (12, 256), 20),
    "pair-8": (8, -32, 16, 100, {"TLSREC_GCM_PAIR_L": "8"}, {"pair_l": 8}, 0, (12, 256), 16),
    "pair-16": (16, -32, 16, 4100, {}, {}, 0, (8, 40), 12),
    "pair-32": (32, -32, 16, 4100, {}, {}, 0, (4, 8), 5),
    "wave-2": (2, -8, 8, 0, {"TLSREC_GCM_WP": "1"}, {"wp": 1}, 2, None, 20),
    "wave-4": (4, -8, 8, 0, {"TLSREC_GCM_WP": "1"}, {"wp": 1}, 4, None, 16),
    "wave-16": (16, -8, 8, 0, {"TLSREC_GCM_WP": "1"}, {"wp": 1}, 16, None, 8),
    "wave-64": (64, -8, 8, 0, {"TLSREC_GCM_WP": "1"}, {"wp": 1}, 64, None, 4),
}
FAMILY_CODES = {(v[0], v[1]) for v in _FAMILIES.values()}
assert len(FAMILY_CODES) == 9


@dataclass(frozen=True)
class Sizing:
    n: int            # records
    nloaded: int      # slots holding a key, the ones without a record included
    rpw: int          # records per wave gcm_plan() returns for it
    tm: int           # GcmArgs::tm it returns


@dataclass(frozen=True)
class Case:
    id: str
    L: int
    code: int
    W: int
    hint: int
    env: dict = field(hash=False, compare=False)
    knobs: dict = field(hash=False, compare=False)
    lanes: int = 0
    band: tuple | None = None
    rpk: int = 0
    cu: int = 0
    runs: Sizing | None = None     # (a): several rounds per wave
    thr: Sizing | None = None      # (b): the smallest n the rule (and the generators) allow

    @property
    def R(self):
        return 64 // self.L

    def plan(self, n, nloaded, nr=14):
        return _abi.gcm_plan(default_knobs(**self.knobs), n=n, nloaded=nloaded, cu=self.cu, avg_bytes=self.hint,
                             lanes=self.lanes, nr=nr, has_cid=0, coalesced=0, keyrun=1)


def edge_values(L):
    s = {0, 1, 15, 16, 17, 1400, 16383}
    for m in (L - 1, L, L + 1, 2 * L, 2 * L + 1):
        s.update(16 * m + d for d in (-1, 0, 1))
    return np.array(sorted(s), dtype=np.uint32)


def min_records(L):
    """the fewest records edge_lengths() can place every value 16 times in"""
    return 4 * 16 * len(edge_values(L))


def case_table(cu):
    """{id: Case}.  The rule's threshold is one full round per wave of a full
    grid, cu x W x R records (for the paired passes tlsrec_plan.h's `n >= cu x
    16 x (64 / Lp)`); thr sits there (raised to what the generators need: 8 |
    n, edge_lengths()'s count), runs is sized upward from it in steps of that
    size until the plan's rpw reaches min(3 R, 64)."""
    out = {}
    for cid, (L, code, W, hint, env, knobs, lanes, band, rpk) in _FAMILIES.items():
        c = Case(cid, L, code, W, hint, env, knobs, lanes, band, rpk, cu)
        R = 64 // L
        step = cu * W * R
        want = min(3 * R, 64)

        def sized(n):
            nloaded = max(2, n // rpk)
            for nr in (10, 14):
                p = c.plan(n, nloaded, nr)
                assert (p.L, p.code) == (L, code), (cid, n, nloaded, nr, p.L, p.code)
            assert band is None or band[0] <= n // nloaded < band[1]
            return Sizing(n, nloaded, int(p.rpw), int(p.tm))

        floor = (max(step, min_records(L)) + 7) // 8 * 8
        thr = sized(floor)
        n = step + 1                       # one record past a full round: the last workgroup holds one record
        while c.plan(n, max(2, n // rpk)).rpw < want:
            n += step
        n = max(n, min_records(L) + 1)
        runs = sized(n)
        assert runs.rpw >= want, (cid, runs)
        out[cid] = Case(cid, L, code, W, hint, env, knobs, lanes, band, rpk, cu, runs, thr)
    return out


# ---- generators -----------------------------------------------------------------
def run_lengths(R):
    """the run lengths every case must hold 8 times: 2, R - 1, R, R + 1, 2 R + 1, without
    values below 1 and duplicates"""
    return [v for v in dict.fromkeys([2, R - 1, R, R + 1, 2 * R + 1]) if v >= 1]


def skewed_counts(nkeys, n, R, rpw, W):
    """records per key, in the pattern's own order (skewed_keyidx shuffles the keys)"""
    special = [v for v in run_lengths(R) for _ in range(8)] + [2 * rpw + 1] * 8 + [W * rpw + 1] * 8
    nz = n1 = -(-nkeys // 16)
    rest = nkeys - len(special) - nz - n1
    left = n - sum(special) - n1
    assert rest >= 4 and left >= rest, f"{n} records over {nkeys} keys leave {left} for {rest} ordinary keys"
    base = left // rest
    h = base // 2
    cnt = base + np.resize(np.array([-h, h, -(h // 2), h // 2], dtype=np.int64), rest)
    diff = left - int(cnt.sum())
    assert abs(diff) <= 2 * rest
    while diff:                         # the remainder, one record at a time over the first keys
        k = min(abs(diff), rest)
        cnt[:k] += 1 if diff > 0 else -1
        diff -= k if diff > 0 else -k
    counts = np.concatenate([np.array(special, dtype=np.int64), np.zeros(nz, np.int64), np.ones(n1, np.int64), cnt])
    assert counts.min() >= 0 and int(counts.sum()) == n and len(counts) == nkeys
    return counts


def check_skew(keyidx, nkeys, R, rpw, W, band):
    """the conditions of a skewed batch, on the slot numbers themselves"""
    n = len(keyidx)
    counts = np.bincount(keyidx, minlength=nkeys)
    assert len(counts) == nkeys
    assert int((counts == 0).sum()) * 16 >= nkeys, "keys without a record"
    assert int((counts == 1).sum()) * 16 >= nkeys, "keys with one record"
    for v in run_lengths(R):
        assert int((counts == v).sum()) >= 8, f"runs of {v}"
    assert int((counts > 2 * rpw).sum()) >= 8, "runs longer than a pair's chunk"
    assert int((counts > W * rpw).sum()) >= 8, "runs longer than a workgroup"
    assert band is None or band[0] <= n // nkeys < band[1], (n // nkeys, band)
    # not round-robin, and not already in key order
    assert len(np.unique(counts)) > 4 and int((np.diff(keyidx.astype(np.int64)) < 0).sum()) > n // 8
    return counts


def skewed_keyidx(nkeys, n, R, rpw, seed, W=16, band=None):
    """slot number of each of n records over nkeys loaded keys"""
    rng = np.random.default_rng(seed)
    counts = skewed_counts(nkeys, n, R, rpw, W)[rng.permutation(nkeys)]
    keyidx = np.repeat(np.arange(nkeys, dtype=np.uint32), counts)[rng.permutation(n)]
    check_skew(keyidx, nkeys, R, rpw, W, band)
    return keyidx


def edge_lengths(L, n, rng):
    """content lengths: a quarter from edge_values(L), every value at least 16
    times and 16383 exactly 16 times, the others uniform in 0..32 L + 64"""
    ev = edge_values(L)
    small = ev[ev != 16383]
    q = n // 4
    assert q - 16 >= 16 * len(small), (L, n)
    lens = rng.integers(0, 32 * L + 65, n).astype(np.uint32)
    lens[rng.permutation(n)[:q]] = np.concatenate([np.resize(small, q - 16), np.full(16, 16383, np.uint32)])
    check_lengths(L, lens)
    return lens


def check_lengths(L, lens):
    vals, cnt = np.unique(lens, return_counts=True)
    have = dict(zip(vals.tolist(), cnt.tolist()))
    for v in edge_values(L).tolist():
        assert have.get(v, 0) >= 16, (L, v, have.get(v, 0))
    assert have[16383] <= 32
    assert int(lens[lens != 16383].max()) <= max(32 * L + 64, 1400, 16 * (2 * L + 1) + 1)


# ---- one case's batch -------------------------------------------------------------
DEC_KINDS = ("tag-bit", "ct-bit", "type", "len-1", "short", "zero-inner", "slot-unloaded", "slot-past")
ENC_KINDS = ("buf-short", "len-16385", "slot-unloaded", "slot-past")
SHORT_LENS = (0, 7, 15, 23)


class RunBatch:
    """n records of one case under (cipher, ver): lens / size / off lay the
    record buffers out in one arena (128-B slots, tag and padding room), slot
    is the key of each record, plain the arena of contents."""

    def __init__(self, case, sizing, cipher, ver, seed, big=None):
        self.case, self.sizing, self.cipher, self.ver = case, sizing, cipher, ver
        n = self.n = sizing.n
        rng = self.rng = np.random.default_rng(seed)
        self.head = 8 if ver == M.VERSION_TLS1_2 else 0
        self.capacity = sizing.nloaded + SPARE_SLOTS
        self.slot = skewed_keyidx(sizing.nloaded, n, case.R, sizing.rpw, seed + 1, case.W, case.band)
        self.lens = edge_lengths(case.L, n, rng)
        room = self.lens.astype(np.uint64)
        if big is not None:               # records whose buffer must hold 16 385 bytes of content
            room[big] = 16385
        self.size = self.head + room + 48
        al = (self.size + 127) // 128 * 128
        self.off = np.zeros(n, dtype=np.uint64)
        self.off[1:] = np.cumsum(al)[:-1]
        self.total = int(self.off[-1] + al[-1])
        self.keys, self.ivs = keys(cipher, sizing.nloaded, rng)
        kl = M.KEYLEN[cipher]
        km = np.zeros(sizing.nloaded, dtype=M.KEY_MATERIAL)
        one = M.key_material(cipher, ver, bytes(kl), bytes(12))[0]
        for f in ("cipher", "tls_minor", "fixed_ivlen", "taglen", "granularity"):
            km[f] = one[f]
        km["key"] = self.keys
        km["iv"][:, :int(one["fixed_ivlen"])] = self.ivs[:, :int(one["fixed_ivlen"])]
        self.km = km
        self.seq = rng.integers(0, 1 << 62, n, dtype=np.uint64)
        self.plain = rng.integers(0, 256, self.total, dtype=np.uint8)
        self.inner = self.lens + 1 + (16 - (self.lens + 1) % 16) % 16 if ver == M.VERSION_TLS1_3 else self.lens
        self.wire = self.head + self.inner + 16
        self._ot = {}

    # descriptors of the good batch
    def desc(self, decrypt):
        d = M.records(self.n)
        d["buf_off"] = self.off
        d["buf_len"] = self.size
        d["data_offset"] = 0 if decrypt else self.head
        d["data_len"] = self.wire if decrypt else self.lens
        d["slot"] = self.slot
        d["ctr"] = M.seq_bytes(self.seq)
        d["type"] = 23
        d["ver"] = (3, 3)
        return d

    def evp(self, mode, plain, got=None, sel=None, nthreads=None):
        """O.evp_check_records over the records sel (all of them when None)"""
        s = slice(None) if sel is None else sel
        return O.evp_check_records(mode, self.cipher, self.ver, self.keys, self.ivs, self.slot[s], self.seq[s],
                                   self.off[s], self.lens[s], plain, got, nthreads or threads())

    def sealed(self):
        """the arena with every record sealed by EVP in place"""
        a = self.plain.copy()
        st = self.evp(0, a)
        assert (st == 0).all()
        return a

    def transform(self, k):
        if k not in self._ot:
            key, iv = bytes(self.keys[k][:M.KEYLEN[self.cipher]]), bytes(self.ivs[k])
            self._ot[k] = O.Transform(self.ver, self.cipher, key, key, iv, iv)
        return self._ot[k]

    def oracle(self, decrypt, d, arena, i):
        """record i of descriptors d over arena through the oracle: (status,
        data_offset, data_len, type, buffer after).  A record naming a slot
        that holds no key never reaches a transform: the ABI's bad-slot result
        (include/tlsrec.h: BAD_INPUT_DATA, the descriptor's fields, the buffer
        untouched)."""
        r = d[i]
        o, size = int(r["buf_off"]), int(r["buf_len"])
        buf = bytearray(arena[o:o + size].tobytes())
        if int(r["slot"]) >= self.sizing.nloaded:
            return (M.ERR_SSL_BAD_INPUT_DATA, int(r["data_offset"]), int(r["data_len"]), int(r["type"]), bytes(buf))
        rec = O.Record(ctr=bytes(r["ctr"]), type=int(r["type"]), ver=bytes(r["ver"]), buf=buf,
                       data_offset=int(r["data_offset"]), data_len=int(r["data_len"]))
        t = self.transform(int(r["slot"]))
        st = t.decrypt_buf(rec) if decrypt else t.encrypt_buf(rec)
        return (st, rec.data_offset, rec.data_len, rec.type, bytes(buf))


def exceptional(n, seed):
    """the n / 8 exceptional records of a batch, at positions of a fixed permutation"""
    assert n % 8 == 0
    return np.random.default_rng(seed).permutation(n)[:n // 8]


def bad_slot(b, kind, j):
    """a slot inside the table that was never loaded / one past its capacity"""
    if kind == "slot-unloaded":
        return b.sizing.nloaded + j % SPARE_SLOTS
    return (b.capacity + j * 7919) if j % 3 else 0xFFFFFFFF


def spoil_decrypt(b, d, arena, ex):
    """make the records ex of the sealed batch (d, arena) exceptional, the
    kinds of DEC_KINDS in rotation; returns each one's kind"""
    kinds = [k for k in DEC_KINDS if k != "zero-inner" or b.ver == M.VERSION_TLS1_3]
    out = []
    for j, i in enumerate(ex.tolist()):
        kind = kinds[j % len(kinds)]
        o, wire, head = int(b.off[i]), int(b.wire[i]), b.head
        if kind == "ct-bit" and b.inner[i] == 0:
            kind = "tag-bit"                     # no ciphertext byte to flip
        if kind == "tag-bit":
            arena[o + wire - 16 + j % 16] ^= 1 << (j % 8)
        elif kind == "ct-bit":
            arena[o + head + (j * 37) % int(b.inner[i])] ^= 1 << (j % 8)
        elif kind == "type":
            d["type"][i] ^= 1 << (j % 3)
        elif kind == "len-1":
            d["data_len"][i] = wire - 1
        elif kind == "short":
            d["data_len"][i] = SHORT_LENS[(j // len(kinds)) % 4]
        elif kind == "zero-inner":
            # content of zeros under type 0, sealed by the oracle: the tag holds, the inner plaintext is all zero
            size = int(b.size[i])
            rec = O.Record(ctr=bytes(d["ctr"][i]), type=0, ver=b"\x03\x03", buf=bytearray(size), data_offset=0,
                           data_len=int(b.lens[i]))
            assert b.transform(int(b.slot[i])).encrypt_buf(rec) == 0 and rec.data_len == wire
            arena[o:o + size] = np.frombuffer(bytes(rec.buf), dtype=np.uint8)
        else:
            d["slot"][i] = bad_slot(b, kind, j)
        out.append(kind)
    return out


def spoil_encrypt(b, d, ex, big):
    """the same for the plaintext batch d, ENC_KINDS in rotation; big: the
    records laid out with room for 16 385 bytes (every fourth of ex, from the
    second)"""
    out = []
    for j, i in enumerate(ex.tolist()):
        kind = ENC_KINDS[j % len(ENC_KINDS)]
        if kind == "buf-short":
            d["buf_len"][i] = int(b.wire[i]) - 1     # head + inner plaintext + tag, less one byte
        elif kind == "len-16385":
            assert big[i]
            d["data_len"][i] = 16385
        else:
            d["slot"][i] = bad_slot(b, kind, j)
        out.append(kind)
    return out


def big_mask(n, ex):
    big = np.zeros(n, dtype=bool)
    big[ex[1::len(ENC_KINDS)]] = True
    return big


def coverage_ok(ver, dec_status, enc_status):
    """the statuses the exceptional records of one case must bring, by the
    oracle: INVALID_MAC on decrypt, BAD_INPUT_DATA on both sides (decrypt: the
    bad-slot result, the only BAD_INPUT_DATA a decrypt has -- ssl_msg.c's
    buffer-bound check returns INTERNAL_ERROR), INVALID_RECORD on TLS 1.3
    decrypt, BUFFER_TOO_SMALL on encrypt"""
    ds, es = set(dec_status), set(enc_status)
    assert M.ERR_SSL_INVALID_MAC in ds and M.ERR_SSL_BAD_INPUT_DATA in ds, ds
    assert ver != M.VERSION_TLS1_3 or M.ERR_SSL_INVALID_RECORD in ds, ds
    assert M.ERR_SSL_BAD_INPUT_DATA in es and M.ERR_SSL_BUFFER_TOO_SMALL in es, es
    assert 0 not in ds and 0 not in es, "an exceptional record the oracle accepts"
    return True


def bad_batches(case, cipher, ver, seed):
    """the two batches of (b) for one case: (b, d, arena, ex, kinds) for
    decrypt (arena sealed, then spoiled) and for encrypt (arena of contents)"""
    ex = exceptional(case.thr.n, seed + 2)
    bd = RunBatch(case, case.thr, cipher, ver, seed)
    dd, arena = bd.desc(True), bd.sealed()
    kd = spoil_decrypt(bd, dd, arena, ex)
    big = big_mask(case.thr.n, ex)
    be = RunBatch(case, case.thr, cipher, ver, seed, big=big)
    de = be.desc(False)
    ke = spoil_encrypt(be, de, ex, big)
    return (bd, dd, arena, ex, kd), (be, de, be.plain.copy(), ex, ke)


# ---- connections with skewed record counts (the stream / DTLS layers) --------------
CONN_PATTERN = (1, 40, 7, 8, 9, 17, 33, 16, 24, 2, 31, 40, 1, 15, 25, 39)


def conn_counts(nrec, nmin=2048):
    """records per connection: CONN_PATTERN over at least nmin connections, at least nrec records"""
    mean = sum(CONN_PATTERN) / len(CONN_PATTERN)
    nconn = max(nmin, int(nrec / mean) + len(CONN_PATTERN))
    counts = np.resize(np.array(CONN_PATTERN), nconn)
    assert counts.sum() >= nrec and (counts == 1).sum() >= 64 and (counts == 40).sum() >= 64
    return counts
