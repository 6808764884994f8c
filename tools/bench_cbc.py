"""Throughput of the AES-CBC + HMAC batch path (device-resident records), with
the AES-128-CCM batch -- the nearest kernel of the same shape: one lane per
record, key passes -- timed in the same run at the same record count and size.

    python tools/bench_cbc.py [--slots 4096] [--steps 5] [--warmup 2] [--out profiles/r07/rows/cbc.jsonl]
                                [--ciphers alt]

One JSON line per (variant, record size, direction): GiB/s of record content.
Decrypt rows read the records the encrypt row of the same variant wrote; both
directions run out of place, so every step sees the same input.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mbedtls_amd as M                    # noqa: E402
from mbedtls_amd import cbc as C           # noqa: E402

VARIANTS = [("cbc128-sha256-mte", C.CIPHER_AES_128_CBC, C.MAC_SHA256, 0),
            ("cbc128-sha256-etm", C.CIPHER_AES_128_CBC, C.MAC_SHA256, 1),
            ("cbc256-sha384-mte", C.CIPHER_AES_256_CBC, C.MAC_SHA384, 0),
            ("cbc128-sha1-mte", C.CIPHER_AES_128_CBC, C.MAC_SHA1, 0),
            ("ccm128", M.CIPHER_AES_128_CCM, 0, 0)]
# --ciphers alt: the ARIA / Camellia suites, each beside its yardsticks -- the AES-CBC row of the same MAC and MAC
# order, and the ARIA- / Camellia-CCM row of the same key size
ALT_VARIANTS = [("cbc128-sha256-mte", C.CIPHER_AES_128_CBC, C.MAC_SHA256, 0),
                ("cbc128-sha256-etm", C.CIPHER_AES_128_CBC, C.MAC_SHA256, 1),
                ("cbc256-sha384-mte", C.CIPHER_AES_256_CBC, C.MAC_SHA384, 0),
                ("cbc256-sha384-etm", C.CIPHER_AES_256_CBC, C.MAC_SHA384, 1)] + \
               [("cbc-%s-%s" % (n, "etm" if e else "mte"), c, C.CBC_ALT_MAC[c], e)
                for n, c in (("aria128-sha256", C.CIPHER_ARIA_128_CBC), ("aria256-sha384", C.CIPHER_ARIA_256_CBC),
                             ("camellia128-sha256", C.CIPHER_CAMELLIA_128_CBC),
                             ("camellia256-sha384", C.CIPHER_CAMELLIA_256_CBC)) for e in (0, 1)] + \
               [("ccm-aria128", M.CIPHER_ARIA_128_CCM, 0, 0), ("ccm-aria256", M.CIPHER_ARIA_256_CCM, 0, 0),
                ("ccm-camellia128", M.CIPHER_CAMELLIA_128_CCM, 0, 0), ("ccm-camellia256", M.CIPHER_CAMELLIA_256_CCM, 0, 0)]
SHAPES = [(1400, 65536), (16384, 8192)]    # content bytes, records
HEAD, ROOM = 16, 16 + 48 + 16              # explicit IV (CCM: 8 of it), MAC / tag and padding


def table(name, cipher, mac, etm, slots, rng):
    kt = M.KeyTable(slots)
    if name.startswith("cbc"):
        km = np.zeros(slots, dtype=C.CBC_KEY_MATERIAL)
        km["cipher"], km["tls_minor"], km["mac"], km["etm"] = cipher, 3, mac, etm
        km["key"] = rng.integers(0, 256, (slots, 32), dtype=np.uint8)
        km["mac_key"] = rng.integers(0, 256, (slots, 48), dtype=np.uint8)
        C.load(kt, km)
    else:
        km = np.concatenate([M.key_material(cipher, M.VERSION_TLS1_2,
                                            bytes(rng.integers(0, 256, M.KEYLEN[cipher], dtype=np.uint8)),
                                            bytes(rng.integers(0, 256, 16, dtype=np.uint8))) for _ in range(slots)])
        kt.load(km)
    return kt


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--ciphers", choices=["aes", "alt"], default="aes",
                    help="aes: the AES-CBC rows and AES-128-CCM; alt: the ARIA / Camellia suites beside their yardsticks")
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda")
    rng = np.random.default_rng(7)
    rows = []
    for name, cipher, mac, etm in (ALT_VARIANTS if args.ciphers == "alt" else VARIANTS):
        kt = table(name, cipher, mac, etm, args.slots, rng)
        for size, n in SHAPES:
            stride = (HEAD + size + ROOM + 127) // 128 * 128
            d = M.records(n)
            d["buf_off"] = np.arange(n, dtype=np.uint64) * stride
            d["buf_len"], d["data_offset"], d["data_len"] = stride, HEAD, size
            d["slot"] = np.arange(n) % args.slots
            d["ctr"] = M.seq_bytes(np.arange(n, dtype=np.uint64))
            d["type"], d["ver"] = 23, np.array([3, 3], dtype=np.uint8)
            plain = torch.randint(0, 256, (n * stride,), dtype=torch.uint8, device=dev)
            sealed = torch.zeros_like(plain)
            opened = torch.zeros_like(plain)
            recs = torch.from_numpy(d.view(np.uint8).copy()).to(dev)
            res = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
            enc_ms = timed(lambda: M.batch_encrypt(kt, recs, res, n, plain, sealed, mean_bytes=stride),
                           args.steps, args.warmup)
            r = res.cpu().numpy().view(M.BATCH_RES)
            assert not r["status"].any(), "encrypt failed"
            d2 = d.copy()
            d2["data_offset"], d2["data_len"], d2["type"] = r["data_offset"], r["data_len"], r["type"]
            recs2 = torch.from_numpy(d2.view(np.uint8).copy()).to(dev)
            dec_ms = timed(lambda: M.batch_decrypt(kt, recs2, res, n, sealed, opened, mean_bytes=stride),
                           args.steps, args.warmup)
            r2 = res.cpu().numpy().view(M.BATCH_RES)
            assert not r2["status"].any() and (r2["data_len"] == size).all(), "decrypt failed"
            for direction, ms in (("encrypt", enc_ms), ("decrypt", dec_ms)):
                row = {"row": name, "direction": direction, "slots": args.slots, "records": n, "content_bytes": size,
                       "ms": round(ms, 4), "gib_per_s": round(n * size / (ms * 1e-3) / 2**30, 2)}
                rows.append(row)
                print(json.dumps(row), flush=True)
        kt.close()
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
