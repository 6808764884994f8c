"""One-key batches for the 16-wave key passes of tlsrec_gcm_kernel (launch
code 16; 8 lanes with the 5-bit Horner table, and 4 lanes), with their
expectation from the oracle record by record.  Test side only; shared by
tests/test_gcm_keypass_phase_cpu.py and tests/test_gcm_keypass_phase_gpu.py.

* count(cu) = cu x 128 + 1 records under one key: gcm_plan() gives 16 records
  per wave at both lane counts, so every wave of a full workgroup is active for
  more than one round, and the last workgroup holds one record -- one wave with
  one busy lane group;
* AEAD lengths at m = 0, 1, L - 1, L, L + 1, 2 L, 2 L + 1 blocks for L = 8 and
  L = 4, each -1 / 0 / +1 byte, in rotation (TLS 1.3: the inner type byte
  counts, padding granularity 1, so no record has 0 bytes), and one record of
  16 383 content bytes in every wave's positions;
* decrypt: the oracle's own seal with one tag in eight corrupted.

gcm_plan() picks 4 lanes for one key only from 16 records per wave of a full
grid (cu x 256); at cu x 128 + 1 the 4-lane key pass is asked for through the
lanes argument of the batch call, and the launch log shows what ran.
"""
from __future__ import annotations

import functools

import numpy as np

import mbedtls_amd as M
import oracle as O
from mbedtls_amd import _abi
from tests import gcmrunlib as G

SUITES, SUITE_IDS = G.SUITES, G.SUITE_IDS
W = 16                    # waves of a key-pass workgroup
RPW = 16                  # records per wave gcm_plan() gives at count(cu), for 8 and 4 lanes
SHAPES = {8: dict(lanes=0, hint=16384), 4: dict(lanes=4, hint=0)}        # L: the batch call's arguments (a hint
#                                                                          goes with the automatic lane choice only)
BIG = 16383
BAD_EVERY, BAD_AT = 8, 3  # record i has its tag corrupted when i % 8 == 3


def count(cu):
    return cu * 128 + 1


def plan(cu, L, cipher):
    a = SHAPES[L]
    return _abi.gcm_plan(G.default_knobs(), n=count(cu), nloaded=1, cu=cu, avg_bytes=a["hint"], lanes=a["lanes"],
                         nr=G.NR[cipher], has_cid=0, coalesced=0, keyrun=1)


def aead_lengths():
    """the AEAD lengths of the edge block counts of both lane counts, sorted"""
    s = set()
    for L in (8, 4):
        for m in (0, 1, L - 1, L, L + 1, 2 * L, 2 * L + 1):
            s.update(16 * m + d for d in (-1, 0, 1) if 16 * m + d >= 0)
    return sorted(s)


def big_positions(n):
    """one record per wave: wave w of workgroup b owns the records b x 256 +
    k x 16 + w, k < 16 (identity order); its big one sits at k = (5 w + b) % 16"""
    i = np.arange(n)
    b, k, w = i // (W * RPW), (i // W) % RPW, i % W
    return np.flatnonzero(k == (5 * w + b) % RPW)


def content_lengths(n, ver):
    inner = 1 if ver == M.VERSION_TLS1_3 else 0
    ev = np.array(aead_lengths(), dtype=np.int64)
    lens = np.maximum(ev[(np.arange(n) * 7) % len(ev)] - inner, 0)     # 7: coprime to the 33 values and to 8
    lens[big_positions(n)] = BIG
    return lens.astype(np.uint32)


class KeyPassBatch:
    """n = count(cu) records of one key under (cipher, ver): the arena of
    contents, the descriptors of both directions, and what the oracle makes of
    each record (fields and the whole buffer)."""

    def __init__(self, cu, cipher, ver, seed):
        self.cu, self.cipher, self.ver = cu, cipher, ver
        n = self.n = count(cu)
        rng = np.random.default_rng(seed)
        self.head = 8 if ver == M.VERSION_TLS1_2 else 0
        self.lens = content_lengths(n, ver)
        self.aead = self.lens + (1 if ver == M.VERSION_TLS1_3 else 0)
        self.wire = self.head + self.aead + 16
        self.size = self.head + self.lens.astype(np.uint64) + 48
        al = (self.size + 127) // 128 * 128
        self.off = np.zeros(n, dtype=np.uint64)
        self.off[1:] = np.cumsum(al)[:-1]
        self.total = int(self.off[-1] + al[-1])
        kl = M.KEYLEN[cipher]
        self.key, self.iv = rng.integers(0, 256, kl, dtype=np.uint8).tobytes(), rng.integers(0, 256, 12, dtype=np.uint8).tobytes()
        self.km = M.key_material(cipher, ver, self.key, self.iv, 1)
        self.ot = O.Transform(ver, cipher, self.key, self.key, self.iv, self.iv, granularity=1)
        self.seq = rng.integers(0, 1 << 62, n, dtype=np.uint64)
        self.plain = rng.integers(0, 256, self.total, dtype=np.uint8)
        self.bad = np.flatnonzero(np.arange(n) % BAD_EVERY == BAD_AT)
        # encrypt: the oracle's seal of every record
        self.enc_desc = self._desc(False)
        self.enc_want, self.enc_out = self._oracle(False, self.enc_desc, self.plain)
        # decrypt: that seal, one tag in eight corrupted
        self.dec_desc = self._desc(True)
        self.dec_in = self.enc_out.copy()
        for j, i in enumerate(self.bad.tolist()):
            self.dec_in[int(self.off[i]) + int(self.wire[i]) - 16 + j % 16] ^= 1 << (j % 8)
        self.dec_want, self.dec_out = self._oracle(True, self.dec_desc, self.dec_in)

    def _desc(self, decrypt):
        d = M.records(self.n)
        d["buf_off"] = self.off
        d["buf_len"] = self.size
        d["data_offset"] = 0 if decrypt else self.head
        d["data_len"] = self.wire if decrypt else self.lens
        d["slot"] = 0
        d["ctr"] = M.seq_bytes(self.seq)
        d["type"] = 23
        d["ver"] = (3, 3)
        return d

    def _oracle(self, decrypt, d, arena):
        """(status, data_offset, data_len, type) of every record and the arena after"""
        want = np.zeros((self.n, 4), dtype=np.int64)
        out = arena.copy()
        for i in range(self.n):
            o, size = int(self.off[i]), int(self.size[i])
            buf = bytearray(arena[o:o + size].tobytes())
            rec = O.Record(ctr=bytes(d["ctr"][i]), type=23, ver=b"\x03\x03", buf=buf,
                           data_offset=int(d["data_offset"][i]), data_len=int(d["data_len"][i]))
            st = self.ot.decrypt_buf(rec) if decrypt else self.ot.encrypt_buf(rec)
            want[i] = (st, rec.data_offset, rec.data_len, rec.type)
            out[o:o + size] = np.frombuffer(bytes(buf), dtype=np.uint8)
        return want, out


@functools.lru_cache(maxsize=None)
def batch(cu, cipher, ver):
    """computed once per suite and shared by the lane counts and directions; read only"""
    b = KeyPassBatch(cu, cipher, ver, 7000 + cipher)
    for a in (b.plain, b.enc_out, b.dec_in, b.dec_out, b.enc_want, b.dec_want):
        a.setflags(write=False)
    return b
