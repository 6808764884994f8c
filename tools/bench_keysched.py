#!/usr/bin/env python3
"""Throughput of the batched key schedules.

Default: TLS 1.3 (tlsrec_tls13_keytab_derive): 64 K connection-direction
traffic secrets in HBM -> KeyUpdate -> write_key / write_iv -> key-table slots
(AES expansion, H, GHASH tables).

--tls12: TLS 1.2 / DTLS 1.2 (tlsrec_tls12_keytab_derive): 64 K connections'
master secret + randoms in HBM -> PRF "key expansion" -> split -> two
key-table slots per connection.  The same run also times
tlsrec_tls13_keytab_derive (no KeyUpdate) for the same number of slots, and a
CPU leg: OpenSSL EVP_KDF "TLS1-PRF" on the host's cores followed by
tlsrec_keytab_load of the result (what a caller without the batch has to do).

Prints one JSON line; the whole call and the derive kernel alone are timed
with HIP events on the call's stream, the key-setup kernel is the difference.

    python tools/bench_keysched.py [--count 65536] [--cipher 2] [--steps 5]
    python tools/bench_keysched.py --tls12 [--prf sha256|sha384] [--count 65536] [--cipher 1]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _cpu_prf_worker(job):
    """One CPU worker's share of the TLS 1.2 CPU leg: EVP_KDF "TLS1-PRF" per
    connection, the key block split into two tlsrec_key_material records
    (64 bytes each; the header is filled by the parent).  Runs in a fresh
    process that never opens the GPU."""
    hname, raw, key_len, iv_len = job
    from tests.tls12_ref import evp_tls1_prf
    need = 2 * key_len + 2 * iv_len
    out = bytearray(len(raw) // 112 * 128)
    t0 = time.perf_counter()
    for i in range(len(raw) // 112):
        c = raw[112 * i:112 * i + 112]
        kb = evp_tls1_prf(hname, c[:48], b"key expansion" + c[48:], need)
        o = 128 * i
        out[o + 32:o + 32 + key_len] = kb[:key_len]
        out[o + 96:o + 96 + key_len] = kb[key_len:2 * key_len]
        out[o + 16:o + 16 + iv_len] = kb[2 * key_len:2 * key_len + iv_len]
        out[o + 80:o + 80 + iv_len] = kb[2 * key_len + iv_len:need]
    return bytes(out), time.perf_counter() - t0


def cpu_tls12_leg(hname, cipher, count, raw, kt):
    """EVP_KDF TLS1-PRF for `count` connections on the host's cores (one
    process per core, ctypes around libcrypto: the per-call Python overhead is
    part of this leg), then tlsrec_keytab_load of the 2 * count records."""
    import multiprocessing as mp
    import torch
    import mbedtls_amd as M
    from bench import host_cores
    threads, how = host_cores()
    kl, il = M.KEYLEN[cipher], 12 if cipher == M.CIPHER_CHACHA20_POLY1305 else 4
    per = (count + threads - 1) // threads
    jobs = [(hname, raw[112 * per * w:112 * per * (w + 1)], kl, il) for w in range(threads)]
    jobs = [j for j in jobs if j[1]]
    with mp.get_context("spawn").Pool(len(jobs)) as pool:
        pool.map(_cpu_prf_worker, [(hname, raw[:112 * 64], kl, il)] * len(jobs))     # start the workers, load libcrypto
        t0 = time.perf_counter()
        parts = pool.map(_cpu_prf_worker, jobs, chunksize=1)
        prf_s = time.perf_counter() - t0
    km = np.frombuffer(b"".join(p for p, _ in parts), dtype=M.KEY_MATERIAL).copy()
    km["cipher"], km["tls_minor"], km["fixed_ivlen"], km["taglen"] = cipher, 3, il, M.TAGLEN[cipher]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    kt.load(km)
    torch.cuda.synchronize()
    load_s = time.perf_counter() - t0
    return {"value": round(count / (prf_s + load_s)), "unit": "connections/s", "cores": threads, "cores_how": how,
            "kind": "evp", "leg": "evp", "prf_seconds": round(prf_s, 4), "keytab_load_seconds": round(load_s, 4),
            "worker_seconds_max": round(max(s for _, s in parts), 4),
            "sample": f"{count} connections: OpenSSL 3 EVP_KDF TLS1-PRF ({hname}) through ctypes in {len(jobs)} "
                      f"processes, then tlsrec_keytab_load of {2 * count} records (host -> device + key setup)"}


def main_tls12(a):
    from tools import rowlib
    import torch
    import mbedtls_amd as M
    from mbedtls_amd import keysched as K
    from mbedtls_amd import tls12 as T
    from mbedtls_amd.batch import _ptr, _stream
    from tests.prng import prng_array
    dev = torch.device("cuda")
    L = M.load()
    vp, u32, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    L.tlsrec__tls12_stage_keys.restype = ci
    L.tlsrec__tls12_stage_keys.argtypes = [vp, u32, u32, ci, ci, vp, vp]
    L.tlsrec__tls13_stage_keys.restype = ci
    L.tlsrec__tls13_stage_keys.argtypes = [vp, u32, u32, ci, vp, ci, vp]
    prf = {"sha256": T.PRF_SHA256, "sha384": T.PRF_SHA384}[a.prf]
    n, nslots = a.count, 2 * a.count
    raw = prng_array(0x7152, n * 112)
    conns = torch.from_numpy(raw).to(dev)
    secrets = torch.from_numpy(prng_array(0x5EC, nslots * 48)).to(dev)
    kt = M.KeyTable(nslots)

    def ok(r):
        assert r == 0, r

    legs = {
        "tls12_call": lambda: T.tls12_keytab_derive(kt, 0, n, a.cipher, prf, conns),
        "tls12_derive_kernel": lambda: ok(L.tlsrec__tls12_stage_keys(kt.handle, 0, n, a.cipher, prf, _ptr(conns),
                                                                      _stream(None))),
        "tls13_call": lambda: K.keytab_derive(kt, 0, nslots, a.cipher, secrets, key_update=False),
        "tls13_derive_kernel": lambda: ok(L.tlsrec__tls13_stage_keys(kt.handle, 0, nslots, a.cipher, _ptr(secrets), 0,
                                                                      _stream(None))),
    }
    ms, wall = {}, {}
    for name, fn in legs.items():
        fn()
        torch.cuda.synchronize()
        ms[name], wall[name] = rowlib.event_timed(fn, a.steps)
    kl, il = M.KEYLEN[a.cipher], 12 if a.cipher == M.CIPHER_CHACHA20_POLY1305 else 4
    per = 112 + 2 * (kl + il)
    cpu = None if a.no_cpu else cpu_tls12_leg(a.prf, a.cipher, n, raw.tobytes(), kt)
    t13_hash = "sha384" if a.cipher == M.CIPHER_AES_256_GCM else "sha256"
    print(json.dumps({
        "metric": "TLS 1.2 key expansions into the key table per second", "value": round(n / (ms["tls12_call"] / 1e3)),
        "unit": "connections/s", "count": n, "slots": nslots, "cipher": a.cipher, "prf": a.prf,
        "ms_per_batch_events": round(ms["tls12_call"], 4), "ms_per_batch_wall": round(wall["tls12_call"] * 1e3, 4),
        "derive_kernel_ms": round(ms["tls12_derive_kernel"], 4),
        "key_setup_ms": round(ms["tls12_call"] - ms["tls12_derive_kernel"], 4),
        "derive_kernel_ns_per_slot": round(ms["tls12_derive_kernel"] * 1e6 / nslots, 3),
        "tls13_same_run": {"slots": nslots, "hash": t13_hash, "key_update": 0,
                           "ms_per_batch_events": round(ms["tls13_call"], 4),
                           "derive_kernel_ms": round(ms["tls13_derive_kernel"], 4),
                           "key_setup_ms": round(ms["tls13_call"] - ms["tls13_derive_kernel"], 4),
                           "derive_kernel_ns_per_slot": round(ms["tls13_derive_kernel"] * 1e6 / nslots, 3)},
        "derive_kernel_speedup_per_slot_vs_tls13": round(ms["tls13_derive_kernel"] / ms["tls12_derive_kernel"], 2),
        "roofline": rowlib.roofline(per * n, ms["tls12_call"], "per connection: the 112-byte tlsrec_tls12_conn read + "
                                    "the two key / IV outputs (2 * (key_len + fixed_ivlen)); the key-table slots the "
                                    "key setup builds are not counted", "tls12 derive + key setup"),
        "cpu_baseline": cpu}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=65536)
    ap.add_argument("--cipher", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--update", type=int, default=1)
    ap.add_argument("--cpu-seconds", type=float, default=2.0, help="wall-time target of the CPU sample")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--tls12", action="store_true", help="the TLS 1.2 key expansion (tlsrec_tls12_keytab_derive)")
    ap.add_argument("--prf", choices=["sha256", "sha384"], default="sha256", help="--tls12: the suite's PRF hash")
    a = ap.parse_args()
    if a.tls12:
        return main_tls12(a)
    from tools import rowlib
    import torch
    import mbedtls_amd as M
    from mbedtls_amd import keysched as K
    from tests.prng import prng_array
    dev = torch.device("cuda")
    secrets = torch.from_numpy(prng_array(0x5EC, a.count * 48)).to(dev)
    kt = M.KeyTable(a.count)
    st = torch.cuda.current_stream()
    K.keytab_derive(kt, 0, a.count, a.cipher, secrets, key_update=bool(a.update))
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
    t0 = time.perf_counter()
    for s, e in ev:
        s.record(st)
        K.keytab_derive(kt, 0, a.count, a.cipher, secrets, key_update=bool(a.update))
        e.record(st)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / a.steps
    ms = float(np.mean([s.elapsed_time(e) for s, e in ev]))
    import oracle as O
    alg = O.SHA384 if a.cipher == 2 else O.SHA256
    keylen = 16 if a.cipher == 1 else 32
    cpu = None if a.no_cpu else rowlib.cpu_keysched_leg(alg, keylen, bool(a.update), a.cpu_seconds)
    # algorithmic bytes per connection: the 48-B secret read (and written back
    # after a KeyUpdate), the key-table slot written -- its 1 KiB state (round
    # keys, H, H powers) and the 70 KiB of GHASH tables the GCM kernels read
    slot = 1024 + (7 * 512 + 26 * 32 + 64) * 16
    per = 48 * (2 if a.update else 1) + slot
    print(json.dumps({"metric": "TLS 1.3 traffic-key derivations into the key table per second",
                      "value": round(a.count / (ms / 1e3)), "unit": "connections/s", "count": a.count,
                      "cipher": a.cipher, "key_update": a.update, "ms_per_batch_events": round(ms, 4),
                      "ms_per_batch_wall": round(wall * 1e3, 4),
                      "roofline": rowlib.roofline(per * a.count, ms, "per connection: secret read (and written after "
                                                  "a KeyUpdate) + the key-table slot written (1 KiB state + 70 KiB "
                                                  "GHASH tables)", "tls13 derive + key setup"),
                      "cpu_baseline": cpu}))


if __name__ == "__main__":
    main()
