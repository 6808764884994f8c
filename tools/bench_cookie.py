#!/usr/bin/env python3
"""DTLS cookie rows (profiles/r16/rows/dtls_cookie.jsonl).

    python tools/bench_cookie.py [--count 65536] [--steps 5] [--id-len 6]

Prints one JSON line per row, all over `count` clients with `id-len`-byte
transport ids (6: an IPv4 address and port), timed with HIP events on the
call's stream (tools/rowlib.event_timed: every kernel of the call, the
fail-closed prefill included):

  batch_write   tlsrec_cookie_batch_write, items/s
  batch_check   tlsrec_cookie_batch_check over the cookies just written
  clihlo        tlsrec_dtls_check_clihlo_cookies over a 50/50 mix of
                ClientHellos with a valid cookie (status 0) and without one
                (HelloVerifyRequest written)
  single_shot   tlsrec_cookie_check, one client per call from host buffers
                (wall time: copies, launch, synchronise): the same box's
                number for a server that does not batch
  cpu           hmac / hashlib on one core of the host: mbedtls_ssl_cookie_check
                restated (tests/cookie_ref.py), for scale only

Each batch row carries ns per SHA-256 compression (2 per item at this id
length: one inner block, one outer) beside the same run's
tlsrec_tls12_batch_verify_data row (PRF-SHA256: 7 per connection), the
word-wise HMAC yardstick of tools/bench_keysched.py --tls12-handshake.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--id-len", type=int, default=6)
    ap.add_argument("--single-shot-calls", type=int, default=2000)
    a = ap.parse_args()

    import torch
    import mbedtls_amd as M
    from mbedtls_amd import cookie as C
    from mbedtls_amd import tls12 as T
    from tests import cookie_ref as R
    from tests.prng import prng_array, prng_bytes
    from tools import rowlib

    dev = torch.device("cuda")
    n, il = a.count, a.id_len
    assert 0 <= il <= 51, "rows are for the one-block case"
    key, now = prng_bytes(0xC0DE, 32), 0x67000000
    ctx = M.CookieContext(key, 60)

    ids = prng_array(0xC1D, n * il).reshape(n, il) if il else np.zeros((n, 0), np.uint8)
    d_ids = torch.from_numpy(ids.reshape(-1).copy() if il else np.zeros(16, np.uint8)).to(dev)
    d_ck = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    st = torch.zeros(n, dtype=torch.int32, device=dev)
    it = np.zeros(n, dtype=C.COOKIE_ITEM)
    it["id_off"] = np.arange(n, dtype=np.uint64) * il
    it["cookie_off"] = np.arange(n, dtype=np.uint64) * 32
    it["id_len"], it["cookie_len"] = il, 32
    d_it = torch.from_numpy(it.view(np.uint8).reshape(-1).copy()).to(dev)

    # ClientHellos: even items echo a valid cookie, odd ones bring none
    idb = [ids[i].tobytes() for i in range(n)]
    head = (bytes([22, 0xfe, 0xfd, 0, 0]) + bytes(6) + bytes(2) + b"\x01" + bytes(3) + bytes(2) + bytes(3) + bytes(3) +
            b"\xfe\xfd" + bytes(32))
    assert len(head) == 59
    tail = b"\x00\x02\xc0\x2b\x01\x00"
    sample = R.cookie_write(key, now, idb[0], 32)[1]
    stride = 128
    arena = np.zeros(n * stride, dtype=np.uint8)
    h = np.zeros(n, dtype=C.CLIHLO)
    d0 = np.frombuffer(head + b"\x00" + b"\x20" + bytes(32) + tail, dtype=np.uint8)
    d1 = np.frombuffer(head + b"\x00" + b"\x00" + tail, dtype=np.uint8)
    rows = arena.reshape(n, stride)
    rows[0::2, :len(d0)] = d0
    rows[1::2, :len(d1)] = d1
    h["off"] = np.arange(n, dtype=np.uint64) * stride
    h["id_off"] = it["id_off"]
    h["out_off"] = np.arange(n, dtype=np.uint64) * 64
    h["len"] = np.where(np.arange(n) % 2 == 0, len(d0), len(d1))
    h["id_len"], h["out_cap"] = il, 64
    d_h = torch.from_numpy(h.view(np.uint8).reshape(-1).copy()).to(dev)
    d_out = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
    res = torch.zeros(n * 8, dtype=torch.uint8, device=dev)

    # the valid cookies come from the write batch itself
    C.batch_write(ctx, now, d_it, n, d_ids, d_ck, st)
    torch.cuda.synchronize()
    cookies = d_ck.cpu().numpy().reshape(n, 32)
    assert cookies[0].tobytes() == sample and int(st.abs().sum().item()) == 0
    rows[0::2, 61:93] = cookies[0::2]
    d_arena = torch.from_numpy(arena).to(dev)

    # the yardstick: tlsrec_tls12_batch_verify_data under PRF-SHA256
    conns = torch.from_numpy(prng_array(0x7158, n * 112)).to(dev)
    trs = torch.from_numpy(prng_array(0x7159, n * 48)).to(dev)
    vd = torch.zeros(n * 16, dtype=torch.uint8, device=dev)

    legs = {
        "batch_write": lambda: C.batch_write(ctx, now, d_it, n, d_ids, d_ck, st),
        "batch_check": lambda: C.batch_check(ctx, now + 1, d_it, n, d_ids, d_ck, st),
        "clihlo": lambda: C.check_clihlo(ctx, now + 1, d_h, n, d_arena, d_ids, d_out, res),
        "verify_data": lambda: T.tls12_batch_verify_data(T.PRF_SHA256, T.IS_CLIENT, conns, trs, None, vd, None, n),
    }
    ms_, wall = {}, {}
    for name, fn in legs.items():
        fn()
        torch.cuda.synchronize()
        ms_[name], wall[name] = rowlib.event_timed(fn, a.steps)
    legs["batch_check"]()
    torch.cuda.synchronize()
    assert int(st.abs().sum().item()) == 0
    r = np.frombuffer(res.cpu().numpy().tobytes(), dtype=C.CLIHLO_RES)
    assert (r["status"][0::2] == 0).all() and (r["status"][1::2] == M.ERR_SSL_HELLO_VERIFY_REQUIRED).all()
    assert (r["olen"][1::2] == 60).all()

    comp = {"batch_write": 2, "batch_check": 2, "clihlo": 2, "verify_data": 7}
    ns = {k: ms_[k] * 1e6 / n / comp[k] for k in comp}
    common = {"count": n, "id_len": il, "steps": a.steps,
              "timing": "HIP events on the call's stream around each timed call (every kernel of the call)",
              "yardstick_same_run": {"call": "tlsrec_tls12_batch_verify_data", "prf": "sha256",
                                     "ms": round(ms_["verify_data"], 4), "compressions_per_connection": 7,
                                     "ns_per_compression": round(ns["verify_data"], 4)}}
    names = {"batch_write": ("tlsrec_cookie_batch_write", "DTLS cookies written per second"),
             "batch_check": ("tlsrec_cookie_batch_check", "DTLS cookies checked per second"),
             "clihlo": ("tlsrec_dtls_check_clihlo_cookies",
                        "DTLS ClientHello datagrams checked per second (half valid, half answered by a "
                        "HelloVerifyRequest)")}
    for k, (call, metric) in names.items():
        print(json.dumps({"row": "dtls_cookie_" + k, "metric": metric, "value": round(n / (ms_[k] / 1e3)),
                          "unit": "items/s", "call": call, "ms_per_batch_events": round(ms_[k], 4),
                          "ms_per_batch_wall": round(wall[k] * 1e3, 4), "compressions_per_item": comp[k],
                          "ns_per_compression": round(ns[k], 4),
                          "per_compression_vs_verify_data_same_run": round(ns[k] / ns["verify_data"], 3), **common}))

    # one client per call, host buffers
    ck = ctx.write(idb[0])[1]
    assert ctx.check(ck, idb[0]) == 0
    t0 = time.perf_counter()
    for _ in range(a.single_shot_calls):
        ctx.check(ck, idb[0])
    single = a.single_shot_calls / (time.perf_counter() - t0)
    t0 = time.perf_counter()
    m = 20000
    for i in range(m):
        R.cookie_check(key, 60, now, sample, idb[0])
    cpu = m / (time.perf_counter() - t0)
    print(json.dumps({"row": "dtls_cookie_single_shot", "metric": "tlsrec_cookie_check calls per second, one thread",
                      "value": round(single), "unit": "items/s", "calls": a.single_shot_calls,
                      "timing": "wall time of the calls: staging copy, one launch, copy back, synchronise",
                      "batch_check_over_single_shot": round(n / (ms_["batch_check"] / 1e3) / single, 1),
                      "cpu_hmac_hashlib_one_core_items_per_s": round(cpu),
                      "cpu_note": "python hmac / hashlib restatement of mbedtls_ssl_cookie_check on one core of the "
                                  "host, interpreter overhead included: for scale, not a tuned CPU baseline"}))
    ctx.close()


if __name__ == "__main__":
    main()
