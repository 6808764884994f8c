"""Record tests/golden/gcm_plan.json: the launch shapes the batch path picks.

    python tests/golden/make_gcm_plan.py [out.json]

Needs the MI355X and the test-hooks library (libtlsrec_test.so).  Every row
loads a key table, issues one encrypt batch of minimal records and reads the
launch log: the AES-GCM entry's (L, waves code, tm), or the ChaCha20-Poly1305
lane count.  The record-size hint is an argument of the call, so the records
stay a few bytes whatever the hint says; a key's records are contiguous, as
the grouped path requires.

The file was recorded once, from the commit before the launch rule moved into
gcm_plan() (csrc/tlsrec_plan.h); tests/test_gcm_plan_cpu.py holds the rule to
it.  Record it again only for a deliberate change of the rule, and review the
diff of the JSON.

A row: path ("lanes" = tlsrec_batch_encrypt with a lane request, "sized" =
tlsrec_batch_encrypt_sized, "grouped" = tlsrec__batch_sized), cipher, nkeys
(keys loaded), n, avg_bytes, lanes, cid, env (the switches set for the row;
every other TLSREC_GCM_* / TLSREC_GROUPED switch unset), cu; then what the log
held: bucket (1 = the bucket pass ran) and L, code, tm (GCM) or L (ChaCha).
"""
from __future__ import annotations

import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import mbedtls_amd as M  # noqa: E402
from mbedtls_amd import _abi  # noqa: E402

G128, G256, G192, CH = M.CIPHER_AES_128_GCM, M.CIPHER_AES_256_GCM, M.CIPHER_AES_192_GCM, M.CIPHER_CHACHA20_POLY1305
KNOBS = ["TLSREC_GCM_WP", "TLSREC_GCM_G5", "TLSREC_GCM_TREEMUL", "TLSREC_GCM_HBUILD", "TLSREC_GCM_PAIR",
         "TLSREC_GROUPED", "TLSREC_GCM_SRECS", "TLSREC_GCM_PAIR_L", "TLSREC_GCM_PAIR_SMALL_MAX",
         "TLSREC_GCM_PAIR_SMALL_MIN", "TLSREC_GCM_PAIR_BIG_MAX", "TLSREC_GCM_LANES"]
STRIDE, HEAD, DATA = 96, 16, 8       # a record: 96 bytes of arena, 8 bytes of content at offset 16


def cases(C):
    """(path, cipher, nkeys, n, avg_bytes, lanes, cid, env) -- one case on each
    side of every threshold of the rule, C = the device's compute units"""
    out = []

    def add(path, cipher, nkeys, n, avg=0, lanes=0, cid=0, **env):
        out.append((path, cipher, nkeys, n, avg, lanes, cid, {"TLSREC_" + k: str(v) for k, v in env.items()}))

    # records per key, no size hint: 2 / 3 (Lfill <= 16), 11 / 12, 47 / 48, 127 / 128
    for k, rpk in ((C * 16, 2), (C * 16, 3), (C * 4, 11), (C * 4, 12), (C * 2, 47), (C * 2, 48), (C * 2, 127),
                   (C * 2, 128)):
        add("sized", G256, k, k * rpk)
    # ... and with a small-record hint: 11 / 12 (PAIR_SMALL_MIN), 127 / 128 (small), 255 / 256 (PAIR_SMALL_MAX)
    for k, rpk in ((C * 16, 11), (C * 16, 12), (C * 4, 127), (C * 4, 128), (C * 4, 255), (C * 4, 256)):
        add("grouped", G256, k, k * rpk, 1400)
        add("sized", G128, k, k * rpk, 1400, GCM_PAIR=0)
    # the hint: unknown, 4096 / 4097, many keys (16 per key) and one key
    for avg in (0, 1, 4096, 4097):
        add("sized", G256, C * 8, C * 128, avg)
        add("sized", G128, 1, C * 256, avg)
    # rpk * avg_bytes either side of 65536 (`light`), where no paired or 4-lane shape applies
    add("sized", G256, 64, 1024, 4095)
    add("sized", G256, 64, 1024, 4096)
    add("grouped", G128, C * 2, C * 64, 2047, GCM_PAIR=0)
    add("grouped", G128, C * 2, C * 64, 2048, GCM_PAIR=0)
    add("sized", G256, C * 4, C * 48, 5461, GCM_PAIR=0)
    add("sized", G256, C * 4, C * 48, 5462, GCM_PAIR=0)
    # n either side of cu*16*2 (Lfill 64 / 16; 3..4 per key), cu*16*8 (Lfill 16 / 8, one key), cu*16*16 (one
    # key, small records: 4 lanes)
    add("sized", G256, C * 8, C * 32 - 1)
    add("sized", G256, C * 8, C * 32)
    add("lanes", G128, 1, C * 32 - 1)
    add("lanes", G128, 1, C * 32)
    add("lanes", G128, 1, C * 128 - 1)
    add("lanes", G128, 1, C * 128)
    add("sized", G256, 1, C * 256 - 1, 1000)
    add("sized", G256, 1, C * 256, 1000)
    # cu*8*16 (small4) and cu*8*32 (small2), the paired passes off
    add("grouped", G256, C * 8, C * 128 - 1, 100, GCM_PAIR=0)
    add("grouped", G256, C * 8, C * 128, 100, GCM_PAIR=0)
    add("grouped", G128, C * 4, C * 256 - 1, 100, GCM_PAIR=0)
    add("grouped", G128, C * 4, C * 256, 100, GCM_PAIR=0)
    # the paired passes: n either side of cu*16*(64/Lp), Lp = 8, 4, 2 (small), 16, 32 (big)
    for k, mult, avg in ((C * 8, 128, 100), (C * 8, 256, 100), (C * 8, 512, 100), (C * 4, 64, 5000),
                         (C * 8, 32, 5000)):
        add("grouped", G256, k, C * mult - 1, avg)
        add("grouped", G256, k, C * mult, avg)
    # big records per key 3 / 4, 7 / 8, 39 / 40
    for k, rpk in ((C * 16, 3), (C * 16, 4), (C * 8, 7), (C * 8, 8), (C * 2, 39), (C * 2, 40)):
        add("grouped", G128, k, k * rpk, 5000)
    # one key on the grouped path (the many-keys shapes apply: few records of one key are wave passes)
    add("grouped", G256, 1, 5, 100)
    add("grouped", G256, 1, C * 256, 100)
    add("grouped", G256, 1, C * 256, 100, GROUPED=0)
    add("sized", G256, 2, 1, 100)
    # AES-128 / 192 / 256 over the shape families
    for c in (G128, G192, G256):
        add("lanes", c, 1, C * 128)
        add("grouped", c, C * 8, C * 32, 200)
        add("grouped", c, C * 8, C * 128, 100)
        add("grouped", c, C * 8, C * 512, 100)
        add("grouped", c, C * 2, C * 128, 100)
    # a table with a connection ID
    add("lanes", G128, 4, 64, cid=1)
    add("sized", G256, C * 8, C * 128, 100, cid=1)
    add("lanes", CH, 4, C * 256, cid=1)
    # explicit lane requests, one key and many keys of few records; TLSREC_GCM_LANES when the caller passes 0
    for lanes in (2, 4, 8, 16, 64, 3):
        add("lanes", G256, 1, C * 32, lanes=lanes)
        add("lanes", G128, C * 8, C * 32, lanes=lanes)
    add("lanes", G256, C * 8, C * 32, GCM_LANES=16)
    add("lanes", G256, C * 8, C * 32, lanes=4, GCM_LANES=16)
    add("sized", G256, C * 8, C * 128, 100, GCM_LANES=3)
    # the switches, over a wave-pass, a small paired and a big paired shape
    shapes = ((C * 8, C * 32, 200), (C * 8, C * 128, 100), (C * 8, C * 64, 5000))
    for env in ({"GCM_WP": 0}, {"GCM_WP": 1}, {"GCM_PAIR": 0}, {"GCM_TREEMUL": 0}, {"GCM_TREEMUL": 1},
                {"GCM_TREEMUL": 7}, {"GCM_HBUILD": 0}, {"GROUPED": 0}, {"GCM_G5": 0}):
        for k, n, avg in shapes:
            add("grouped", G256, k, n, avg, **env)
    add("lanes", G128, C * 2, C * 128, GCM_WP=1)             # 64 per key: wave passes only when forced
    add("lanes", G128, 1, C * 128, GCM_WP=1)
    add("lanes", G128, 1, C * 128, GCM_TREEMUL=0)
    for v in (2, 4, 8, 16):                                   # (16: not a lane count of the small paired passes)
        add("grouped", G256, C * 8, C * 512, 100, GCM_PAIR_L=v)
    add("grouped", G256, C * 8, C * 64, 5000, GCM_PAIR_L=8)   # (the override is for small records only)
    add("grouped", G128, C * 8, C * 128, 100, GCM_PAIR_SMALL_MIN=17)
    add("grouped", G128, C * 8, C * 128, 100, GCM_PAIR_SMALL_MAX=16)
    add("grouped", G128, C * 2, C * 512, 100, GCM_PAIR_SMALL_MAX=300)
    add("grouped", G128, C * 8, C * 128, 5000, GCM_PAIR_BIG_MAX=16)
    add("grouped", G128, C * 2, C * 100, 5000, GCM_PAIR_BIG_MAX=64)
    # ChaCha20-Poly1305: n either side of cu*8*16 and cu*8*32, the lane requests
    for n in (C * 128 - 1, C * 128, C * 256 - 1, C * 256):
        add("grouped", CH, 64, n, 100)
    for lanes in (1, 2, 4, 8, 16):
        add("lanes", CH, 4, C * 64, lanes=lanes)
    return out


class Recorder:
    def __init__(self):
        self.lib = _abi.test_library()
        self.lib.tlsrec__batch_sized.restype = ctypes.c_int
        self.lib.tlsrec__batch_sized.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint32] + [ctypes.c_void_p] * 3 + \
            [ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_int]
        self.dev = torch.device("cuda")
        self.cu = torch.cuda.get_device_properties(0).multi_processor_count
        self.tables = {}
        self.nmax = 0

    def reserve(self, nmax):
        self.nmax = nmax
        self.arena = torch.zeros(nmax * STRIDE, dtype=torch.uint8, device=self.dev)
        self.res = torch.zeros(nmax * 16, dtype=torch.uint8, device=self.dev)
        self.recs = torch.zeros(nmax * 40, dtype=torch.uint8, device=self.dev)

    def table(self, cipher, nkeys, cid):
        key = (cipher, nkeys, cid)
        if key not in self.tables:
            km = np.zeros(nkeys, dtype=_abi.KEY_MATERIAL)
            km["cipher"] = cipher
            # DTLS 1.2 keys for the table with a connection ID, else TLS 1.3
            km["tls_minor"] = 3 if cid else 4
            km["fixed_ivlen"] = 4 if (cid and cipher != CH) else 12
            km["taglen"] = 16
            rng = np.random.default_rng(1000 * cipher + nkeys)
            km["iv"][:, :12] = rng.integers(0, 256, (nkeys, 12), dtype=np.uint8)
            km["key"][:, :M.KEYLEN[cipher]] = rng.integers(0, 256, (nkeys, M.KEYLEN[cipher]), dtype=np.uint8)
            kt = M.KeyTable(nkeys)
            kt.load(km)
            if cid:
                kt.set_cid(0, b"\xc1\xd2\xe3")
            self.tables[key] = kt
        return self.tables[key]

    def run(self, path, cipher, nkeys, n, avg, lanes, cid, env):
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env)
        kt = self.table(cipher, nkeys, cid)
        d = M.records(n)
        i = np.arange(n, dtype=np.uint64)
        d["buf_off"], d["buf_len"], d["data_offset"], d["data_len"] = i * STRIDE, STRIDE, HEAD, DATA
        d["slot"] = (i * nkeys // n).astype(np.uint32)          # a key's records together
        d["ctr"] = M.seq_bytes(i + 1)
        d["type"] = 23
        d["ver"][:] = (0xFE, 0xFD) if cid else (3, 3)
        self.recs[:n * 40] = torch.from_numpy(d.view(np.uint8).copy()).to(self.dev)
        torch.cuda.synchronize()
        st = torch.cuda.current_stream().cuda_stream
        _abi.launch_log_reset()
        p = (kt.handle, self.recs.data_ptr(), self.res.data_ptr(), n, self.arena.data_ptr(), self.arena.data_ptr())
        if path == "lanes":
            rc = self.lib.tlsrec_batch_encrypt(*p, lanes, st)
        elif path == "sized":
            rc = self.lib.tlsrec_batch_encrypt_sized(*p, avg, st)
        else:
            rc = self.lib.tlsrec__batch_sized(*p, st, 0, avg, 0, 0)
        torch.cuda.synchronize()
        assert rc == 0, (rc, path, cipher, nkeys, n)
        log = _abi.launch_log_read()
        for k in env:
            os.environ.pop(k, None)
        row = {"path": path, "cipher": cipher, "nkeys": nkeys, "n": n, "avg_bytes": avg, "lanes": lanes, "cid": cid,
               "env": env, "cu": self.cu, "bucket": [e[1] for e in log if e[0] == _abi.LOG_BUCKET][0]}
        if cipher == CH:
            (e,) = [e for e in log if e[0] == _abi.LOG_CHACHA]
            row.update(L=e[1])
        else:
            (e,) = [e for e in log if e[0] == _abi.LOG_GCM]
            row.update(L=e[1], code=e[2], tm=e[3])
        return row


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "gcm_plan.json")
    assert "TLSREC_GCM_WAVES" not in os.environ
    with _abi.use_library():
        r = Recorder()
        cs = cases(r.cu)
        r.reserve(max(c[3] for c in cs))
        rows = [r.run(*c) for c in cs]
        for kt in r.tables.values():
            kt.close()
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(row) for row in rows) + "\n]\n")
    print(len(rows), "rows ->", out)


if __name__ == "__main__":
    main()
