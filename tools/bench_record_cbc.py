"""Latency of the single-record calls on a CBC + HMAC transform: one thread,
AES-128-CBC + HMAC-SHA256, both MAC orders, 1 400 and 16 384 content bytes.

    python tools/bench_record_cbc.py [--calls 400] [--warmup 40] [--out profiles/r12/rows/record_cbc.jsonl]

One JSON line per (direction, MAC order, size, kernel, leg): p50 and p99 of
tlsrec_decrypt_buf / tlsrec_encrypt_buf in microseconds.  The decrypt rows are
taken twice in one process, alternating A B B A: A is TLSREC_CBC_WAVE=0 (the
lane kernel reached through the single-record path), B the wave-per-record
kernel.  A last line states the decision rule's inputs and outcome: the wave
kernel is the default only if its 16 KiB p50 is below the lane kernel's by more
than the lane kernel's own two legs differ, and its 1 400 B p50 is not above the
lane kernel's by more than that same difference.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mbedtls_amd as M                    # noqa: E402
from mbedtls_amd import _abi               # noqa: E402

SIZES = (1400, 16384)
ROOM = 16 + 32 + 16


def timed(fn, make, calls, warmup):
    us = []
    for i in range(warmup + calls):
        rec = make()
        t0 = time.perf_counter_ns()
        st = fn(rec)
        t1 = time.perf_counter_ns()
        assert st == 0, st
        if i >= warmup:
            us.append((t1 - t0) / 1e3)
    return float(np.percentile(us, 50)), float(np.percentile(us, 99))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--out", default=os.path.join("profiles", "r12", "rows", "record_cbc.jsonl"))
    a = ap.parse_args()
    rng = np.random.default_rng(12)
    rows = []
    for etm in (0, 1):
        key, mac = bytes(rng.integers(0, 256, 16, dtype=np.uint8)), bytes(rng.integers(0, 256, 32, dtype=np.uint8))
        t = M.Transform.cbc(M.VERSION_TLS1_2, _abi.CIPHER_AES_128_CBC, _abi.MAC_SHA256, etm, key, key, mac, mac)
        for n in SIZES:
            content = bytes(rng.integers(0, 256, n, dtype=np.uint8))

            def plain():
                return M.Record(ctr=bytes(8), type=23, ver=b"\x03\x03", buf=bytearray(16) + bytearray(content) +
                                bytearray(ROOM), data_offset=16, data_len=n)
            sealed = plain()
            assert t.encrypt_buf(sealed) == 0
            wire, off, ln = bytes(sealed.buf), sealed.data_offset, sealed.data_len

            def cipher():
                return M.Record(ctr=bytes(8), type=23, ver=b"\x03\x03", buf=bytearray(wire), data_offset=off, data_len=ln)
            p50, p99 = timed(t.encrypt_buf, plain, a.calls, a.warmup)
            rows.append({"call": "encrypt_buf", "etm": etm, "bytes": n, "kernel": "lane", "leg": 0, "p50_us": p50,
                         "p99_us": p99})
            for leg, knob in enumerate(("0", "1", "1", "0")):           # A B B A
                os.environ["TLSREC_CBC_WAVE"] = knob
                p50, p99 = timed(t.decrypt_buf, cipher, a.calls, a.warmup)
                rows.append({"call": "decrypt_buf", "etm": etm, "bytes": n, "kernel": "wave" if knob == "1" else "lane",
                             "leg": leg, "p50_us": p50, "p99_us": p99})
            del os.environ["TLSREC_CBC_WAVE"]
        t.close()
    # the rule, per MAC order: the mean p50 of each kernel's two legs, the lane kernel's leg-to-leg difference
    verdicts = []
    for etm in (0, 1):
        v = {"etm": etm}
        for n in SIZES:
            leg = {k: [r["p50_us"] for r in rows if r["call"] == "decrypt_buf" and r["etm"] == etm and r["bytes"] == n
                       and r["kernel"] == k] for k in ("lane", "wave")}
            v[n] = {"lane_p50": sum(leg["lane"]) / 2, "wave_p50": sum(leg["wave"]) / 2,
                    "lane_leg_diff": abs(leg["lane"][0] - leg["lane"][1])}
        big, small = v[16384], v[1400]
        v["wave_default"] = bool(big["lane_p50"] - big["wave_p50"] > big["lane_leg_diff"] and
                                 small["wave_p50"] - small["lane_p50"] <= small["lane_leg_diff"])
        verdicts.append({"etm": etm, "p50": {str(n): v[n] for n in SIZES}, "wave_default": v["wave_default"]})
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
        f.write(json.dumps({"decision": verdicts, "wave_default": all(v["wave_default"] for v in verdicts),
                            "calls": a.calls, "version": M.version()}) + "\n")
    for r in rows:
        print(json.dumps(r))
    print(json.dumps({"decision": verdicts}))


if __name__ == "__main__":
    main()
