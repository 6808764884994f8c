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

--tls12 --cbc-mac {1,2,3} [--etm]: the AES-CBC + HMAC suites
(tlsrec_tls12_keytab_derive_cbc) at the suite shape of the MAC -- 1: AES-128-CBC
SHA-1 with PRF SHA-256, 2: AES-128-CBC SHA-256 with PRF SHA-256, 3: AES-256-CBC
SHA-384 with PRF SHA-384 (--cipher 23|24 and --prf override).  One run times
(a) the call, (b) its derive kernel alone, (c) the host path it replaces --
tlsrec_tls12_make_keys_cbc per connection, then one tlsrec_keytab_load_cbc --
on a sample of at most 2 048 connections, and (d) tlsrec_tls12_keytab_derive
for AES-128-GCM over the same connections as the yardstick, and states the
derive kernels' cost per SHA-2 compression (DESIGN 3.5's 5n + 3 / 5n + 2).

--tls13-handshake: the TLS 1.3 ladder (tlsrec_tls13_keytab_derive_handshake,
_application, tlsrec_tls13_batch_verify_data, _batch_derive_secret) over 64 K
connections of one (cipher, psk_len, shared_len): each call, each stage's
derive kernel alone, the single-shot ladder + tlsrec_keytab_load it replaces
on at most 2 048 connections, and the tlsrec_tls12_keytab_derive AES-128-GCM
kernel under the same hash for a ns-per-compression yardstick.

--tls13-early: a resumed handshake's batches over 64 K connections of one
(cipher, psk_len): tlsrec_tls13_keytab_derive_early (--no-keys:
tlsrec_tls13_batch_psk_binder), its derive kernel alone, the binder-only kernel,
tlsrec_tls13_batch_ticket_psk, the host path it replaces on at most 2 048
connections (create_psk_binder + derive_early_secrets + make_traffic_keys per
connection, then one tlsrec_keytab_load), and the handshake-stage derive kernel
under the same hash for the ns-per-compression yardstick.

--tls12-handshake: the TLS 1.2 / DTLS 1.2 handshake batches over 64 K connections
of one (prf, pms_len, extended_ms): (a) tlsrec_tls12_batch_compute_master, (b) the
chain compute_master -> tlsrec_tls12_keytab_derive (AES-128-GCM under SHA-256,
AES-256-GCM under SHA-384) as one enqueue, (c) tlsrec_tls12_batch_verify_data
with offered values, (d) the host path they replace on at most 2 048
connections (tlsrec_tls12_compute_master + tlsrec_tls12_calc_finished per
connection), and (e) the tlsrec_tls12_keytab_derive AES-128-GCM derive kernel
under the same hash for the ns-per-compression yardstick.

--exporter: the exporter batches (tlsrec_tls13_batch_exporter,
tlsrec_tls12_batch_export_keying_material) over 64 K connections under one hash
at three shapes -- DTLS-SRTP ("EXTRACTOR-dtls_srtp", no context, 60 bytes),
EAP-TLS ("EXPORTER_EAP_TLS_Key_Material", a shared 1-byte context, 128 bytes),
channel binding ("EXPORTER-Channel-Binding", no context, 32 bytes): each call,
the single-shot call it replaces on at most 2 048 connections, and the
tlsrec_tls12_keytab_derive AES-128-GCM derive kernel under the same hash for the
ns-per-compression yardstick (exporters).  One JSON line per (version, shape).

--x25519: the key exchange in front of all of the above (tlsrec_x25519_batch_public,
tlsrec_x25519_batch_shared): (a) and (b) the two calls alone at 4 096, 65 536 and 1 048 576
connections, (c) the chain batch_shared -> tlsrec_tls13_keytab_derive_handshake
(AES-128-GCM, no PSK) as one enqueue at --count connections, with the share of it that is
the key exchange, and (d) the CPU path it replaces: OpenSSL EVP_PKEY_derive, one worker
process per CPU of the share (at most 16), with one context, timing the derive alone
(through ctypes).  One JSON line per leg.

Prints one JSON line; the whole call and the derive kernel alone are timed
with HIP events on the call's stream, the key-setup kernel is the difference.

    python tools/bench_keysched.py [--count 65536] [--cipher 2] [--steps 5]
    python tools/bench_keysched.py --tls12 [--prf sha256|sha384] [--count 65536] [--cipher 1]
    python tools/bench_keysched.py --tls12 --cbc-mac 2 [--etm] [--count 65536]
    python tools/bench_keysched.py --tls13-handshake [--cipher 1|2] [--psk-len 32] [--shared-len 32]
    python tools/bench_keysched.py --tls13-early [--cipher 1|2|3] [--psk-len 32] [--no-keys]
    python tools/bench_keysched.py --tls12-handshake [--prf sha256|sha384] [--pms-len 32] [--ems]
    python tools/bench_keysched.py --exporter [--prf sha256|sha384]
    python tools/bench_keysched.py --x25519 [--count 65536]
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


def _compressions(hname, out_len):
    """SHA-2 compressions of one connection's key expansion: 5n + 3 (SHA-256), 5n + 2 (SHA-384)"""
    h, extra = (48, 2) if hname == "sha384" else (32, 3)
    return 5 * ((out_len + h - 1) // h) + extra


def host_cbc_leg(prf, cipher, mac, etm, raw, sample):
    """The path without the batch: tlsrec_tls12_make_keys_cbc per connection (a
    synchronised single-shot PRF job each, the keys returned to the host), then
    one tlsrec_keytab_load_cbc of the 2 * sample records."""
    import torch
    import mbedtls_amd as M
    from mbedtls_amd import cbc as C
    kt = M.KeyTable(2 * sample)
    C.make_keys(prf, cipher, mac, raw[:48], raw[48:112])          # the control-path stream and arena exist
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    parts = []
    for i in range(sample):
        st, cw, sw = C.make_keys(prf, cipher, mac, raw[112 * i:112 * i + 48], raw[112 * i + 48:112 * i + 112])
        assert st == 0, st
        parts += [cw, sw]
    keys = np.concatenate(parts)
    keys["etm"] = etm
    make_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    C.load(kt, keys)
    torch.cuda.synchronize()
    load_s = time.perf_counter() - t0
    kt.close()
    tot = make_s + load_s
    return {"value": round(sample / tot), "unit": "connections/s", "sample_connections": sample,
            "us_per_connection": round(tot / sample * 1e6, 2), "make_keys_seconds": round(make_s, 4),
            "keytab_load_cbc_seconds": round(load_s, 4),
            "what": "tlsrec_tls12_make_keys_cbc per connection (one synchronised PRF job each, keys to the host), "
                    "then one tlsrec_keytab_load_cbc (keys back to the device + key setup); wall time"}


def main_tls12_cbc(a):
    from tools import rowlib
    import torch
    import mbedtls_amd as M
    from mbedtls_amd import cbc as C
    from mbedtls_amd import tls12 as T
    from mbedtls_amd.batch import _ptr, _stream
    from tests.prng import prng_array
    dev = torch.device("cuda")
    L = M.load()
    vp, u32, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    L.tlsrec__tls12_stage_keys.restype = ci
    L.tlsrec__tls12_stage_keys.argtypes = [vp, u32, u32, ci, ci, vp, vp]
    L.tlsrec__tls12_stage_keys_cbc.restype = ci
    L.tlsrec__tls12_stage_keys_cbc.argtypes = [vp, u32, u32, ci, ci, ci, ci, vp, vp]
    mac, etm = a.cbc_mac, int(a.etm)
    cipher = a.cipher if a.cipher is not None else (C.CIPHER_AES_256_CBC if mac == C.MAC_SHA384 else C.CIPHER_AES_128_CBC)
    hname = a.prf or ("sha384" if mac == C.MAC_SHA384 else "sha256")
    prfs = {"sha256": T.PRF_SHA256, "sha384": T.PRF_SHA384}
    prf, gcm = prfs[hname], M.CIPHER_AES_128_GCM
    n, nslots = a.count, 2 * a.count
    raw = prng_array(0x7152, n * 112)
    conns = torch.from_numpy(raw).to(dev)
    kt, kt_gcm = M.KeyTable(nslots), M.KeyTable(nslots)     # a table each: no reload wipes in the timed calls

    def ok(r):
        assert r == 0, r

    # the derive kernel alone leaves raw keys staged; the call that follows it zeroizes the range
    legs = {
        "cbc_derive_kernel": lambda: ok(L.tlsrec__tls12_stage_keys_cbc(kt.handle, 0, n, cipher, mac, etm, prf,
                                                                        _ptr(conns), _stream(None))),
        "cbc_call": lambda: T.tls12_keytab_derive_cbc(kt, 0, n, cipher, mac, etm, prf, conns),
        "gcm_derive_kernel": lambda: ok(L.tlsrec__tls12_stage_keys(kt_gcm.handle, 0, n, gcm, T.PRF_SHA256, _ptr(conns),
                                                                   _stream(None))),
        "gcm_call": lambda: T.tls12_keytab_derive(kt_gcm, 0, n, gcm, T.PRF_SHA256, conns),
    }
    if hname == "sha384":       # the AEAD kernel under the same hash: SHA-512 compressions against SHA-512 ones
        legs["gcm384_derive_kernel"] = lambda: ok(L.tlsrec__tls12_stage_keys(kt_gcm.handle, 0, n, gcm, T.PRF_SHA384,
                                                                             _ptr(conns), _stream(None)))
    ms, wall = {}, {}
    for name, fn in legs.items():
        fn()
        torch.cuda.synchronize()
        ms[name], wall[name] = rowlib.event_timed(fn, a.steps)
    legs["gcm_call"]()          # (the SHA-384 kernel leg staged keys the table never took)
    torch.cuda.synchronize()
    kl, ml = C.CBC_ALL_KEYLEN[cipher], C.MACLEN[mac]
    out_len = 2 * ml + 2 * kl
    comp = {"cbc": _compressions(hname, out_len), "gcm": _compressions("sha256", 40), "gcm384": _compressions("sha384", 40)}
    ns = {k: ms[k + "_derive_kernel"] * 1e6 / n / comp[k] for k in comp if k + "_derive_kernel" in ms}
    has384 = "gcm384" in ns
    host = None if a.no_cpu else host_cbc_leg(prf, cipher, mac, etm, raw.tobytes(), min(2048, n))
    call_cps = n / (ms["cbc_call"] / 1e3)
    print(json.dumps({
        "metric": "TLS 1.2 CBC + HMAC key expansions into the key table per second", "value": round(call_cps),
        "unit": "connections/s", "count": n, "slots": nslots, "cipher": cipher, "mac": mac, "etm": etm, "prf": hname,
        "key_block_bytes": out_len, "compressions_per_connection": comp["cbc"],
        "ms_per_batch_events": round(ms["cbc_call"], 4), "ms_per_batch_wall": round(wall["cbc_call"] * 1e3, 4),
        "derive_kernel_ms": round(ms["cbc_derive_kernel"], 4),
        "key_setup_and_wipe_ms": round(ms["cbc_call"] - ms["cbc_derive_kernel"], 4),
        "key_setup_share_of_call": round(1 - ms["cbc_derive_kernel"] / ms["cbc_call"], 4),
        "derive_kernel_ns_per_connection": round(ms["cbc_derive_kernel"] * 1e6 / n, 3),
        "derive_kernel_ns_per_compression": round(ns["cbc"], 4),
        "aes128gcm_same_run": {"prf": "sha256", "connections_per_s": round(n / (ms["gcm_call"] / 1e3)),
                               "ms_per_batch_events": round(ms["gcm_call"], 4),
                               "derive_kernel_ms": round(ms["gcm_derive_kernel"], 4),
                               "key_setup_ms": round(ms["gcm_call"] - ms["gcm_derive_kernel"], 4),
                               "compressions_per_connection": comp["gcm"],
                               "derive_kernel_ns_per_compression": round(ns["gcm"], 4),
                               "prf_sha384_derive_kernel_ms": round(ms["gcm384_derive_kernel"], 4) if has384 else None,
                               "prf_sha384_compressions_per_connection": comp["gcm384"] if has384 else None,
                               "prf_sha384_derive_kernel_ns_per_compression": round(ns["gcm384"], 4) if has384 else None},
        "per_compression_vs_aead_kernel_same_hash": round(ns["cbc"] / ns["gcm384" if hname == "sha384" else "gcm"], 3),
        "per_compression_vs_aes128gcm_sha256": round(ns["cbc"] / ns["gcm"], 3),
        "host_path": host,
        "speedup_vs_host_path": round(call_cps / host["value"], 1) if host else None,
        "roofline": rowlib.roofline((112 + out_len) * n, ms["cbc_call"], "per connection: the 112-byte tlsrec_tls12_conn "
                                    "read + the key block (2 * (maclen + key_len)); the key-table slots the key setup "
                                    "builds are not counted", "tls12 cbc derive + cbc key setup + staging wipe")}))


def host_tls13_ladder_leg(hash_alg, cipher, psk_len, shared_len, raw, traw, sample):
    """The path without the batch, for `sample` connections: the single-shot
    ladder per connection (a synchronised job chain per step, every secret back
    on the host), then one tlsrec_keytab_load per stage."""
    import torch
    import mbedtls_amd as M
    from mbedtls_amd import keysched as K
    H, kl = K.HASH_LEN[hash_alg], M.KEYLEN[cipher]
    kt = M.KeyTable(2 * sample)
    K.evolve_secret(hash_alg, None, None)                        # the control-path stream and arena exist

    def load(pairs):
        km = np.concatenate([M.key_material(cipher, M.VERSION_TLS1_3, k, iv) for k, iv in pairs])
        t0 = time.perf_counter()
        kt.load(km)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pairs, masters = [], []
    for i in range(sample):
        c = raw[176 * i:176 * i + 176]
        early = K.evolve_secret(hash_alg, None, c[:psk_len] or None)
        hs = K.evolve_secret(hash_alg, early, c[48:48 + shared_len] or None)
        cs, ss = K.derive_handshake_secrets(hash_alg, hs, c[128:128 + H])
        ck, civ, sk, siv = K.make_traffic_keys(hash_alg, cs, ss, kl, 12)
        for s in (cs, ss):
            K.hkdf_expand_label(hash_alg, s, b"finished", b"", H)
        masters.append(K.evolve_secret(hash_alg, hs, None))
        pairs += [(ck, civ), (sk, siv)]
    hs_s = time.perf_counter() - t0
    hs_load = load(pairs)
    t0 = time.perf_counter()
    pairs = []
    for i in range(sample):
        ca, sa, _ = K.derive_application_secrets(hash_alg, masters[i], traw[48 * i:48 * i + H])
        ck, civ, sk, siv = K.make_traffic_keys(hash_alg, ca, sa, kl, 12)
        pairs += [(ck, civ), (sk, siv)]
    app_s = time.perf_counter() - t0
    app_load = load(pairs)
    kt.close()

    def row(ladder, ld):
        return {"value": round(sample / (ladder + ld)), "unit": "connections/s",
                "us_per_connection": round((ladder + ld) / sample * 1e6, 2), "ladder_seconds": round(ladder, 4),
                "keytab_load_seconds": round(ld, 4)}
    return {"sample_connections": sample, "handshake": row(hs_s, hs_load), "application": row(app_s, app_load),
            "what": "per connection the single-shot calls (handshake: evolve_secret x3, derive_handshake_secrets, "
                    "make_traffic_keys, hkdf_expand_label \"finished\" x2; application: derive_application_secrets, "
                    "make_traffic_keys), then one tlsrec_keytab_load of the stage's records; wall time"}


def main_tls13_handshake(a):
    """tlsrec_tls13_keytab_derive_handshake / _application and the two table-less
    batches: each call, each stage's derive kernel alone, the host path they
    replace, and the TLS 1.2 AES-128-GCM derive kernel of the same run under
    the same hash as the ns-per-compression yardstick."""
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
    L.tlsrec__tls13_stage_hs_keys.restype = ci
    L.tlsrec__tls13_stage_hs_keys.argtypes = [vp, u32, u32, ci, u32, u32, vp, vp, vp, vp, vp]
    L.tlsrec__tls13_stage_app_keys.restype = ci
    L.tlsrec__tls13_stage_app_keys.argtypes = [vp, u32, u32, ci, vp, vp, vp, vp, vp]
    L.tlsrec__tls12_stage_keys.restype = ci
    L.tlsrec__tls12_stage_keys.argtypes = [vp, u32, u32, ci, ci, vp, vp]
    cipher, pl, sl, n = a.cipher, a.psk_len, a.shared_len, a.count
    sha384 = cipher == M.CIPHER_AES_256_GCM
    hname, alg = ("sha384", K.ALG_SHA_384) if sha384 else ("sha256", K.ALG_SHA_256)
    raw, traw = prng_array(0x7153, n * 176), prng_array(0x7154, n * 48)
    conns, trs = torch.from_numpy(raw).to(dev), torch.from_numpy(traw).to(dev)
    conns12 = torch.from_numpy(prng_array(0x7152, n * 112)).to(dev)

    def buf(k):
        return torch.zeros(k * 48, dtype=torch.uint8, device=dev)

    hs, fin, ms, app, exp, vd, rm = buf(2 * n), buf(2 * n), buf(n), buf(2 * n), buf(n), buf(2 * n), buf(n)
    kt, kt12 = M.KeyTable(2 * n), M.KeyTable(2 * n)
    prf12 = T.PRF_SHA384 if sha384 else T.PRF_SHA256

    def ok(r):
        assert r == 0, r

    s = _stream(None)
    legs = {
        "hs_call": lambda: K.keytab_derive_handshake(kt, 0, n, cipher, pl, sl, conns, hs, fin, ms),
        "hs_derive_kernel": lambda: ok(L.tlsrec__tls13_stage_hs_keys(kt.handle, 0, n, cipher, pl, sl, _ptr(conns), _ptr(hs),
                                                                      _ptr(fin), _ptr(ms), s)),
        "app_call": lambda: K.keytab_derive_application(kt, 0, n, cipher, ms, trs, app, exp),
        "app_derive_kernel": lambda: ok(L.tlsrec__tls13_stage_app_keys(kt.handle, 0, n, cipher, _ptr(ms), _ptr(trs),
                                                                        _ptr(app), _ptr(exp), s)),
        "verify_data": lambda: K.batch_verify_data(alg, fin, hs, vd, 2 * n),
        "derive_secret": lambda: K.batch_derive_secret(alg, b"res master", ms, trs, rm, n),
        "tls12_derive_kernel": lambda: ok(L.tlsrec__tls12_stage_keys(kt12.handle, 0, n, M.CIPHER_AES_128_GCM, prf12,
                                                                     _ptr(conns12), s)),
    }
    ms_, wall = {}, {}
    for name, fn in legs.items():
        fn()
        torch.cuda.synchronize()
        ms_[name], wall[name] = rowlib.event_timed(fn, a.steps)
    legs["app_call"]()          # (the kernel-alone legs staged keys the table never took)
    torch.cuda.synchronize()
    comp = {"hs": (8 if pl else 0) + (3 if not sha384 and sl > 55 else 2) + 2 + 4 + 6 + 16, "app": 20,
            "verify_data": 4, "derive_secret": 4, "tls12": _compressions(hname, 40)}
    per = {"hs": n, "app": n, "verify_data": 2 * n, "derive_secret": n, "tls12": n}
    leg = {"hs": "hs_derive_kernel", "app": "app_derive_kernel", "verify_data": "verify_data",
           "derive_secret": "derive_secret", "tls12": "tls12_derive_kernel"}
    ns = {k: ms_[leg[k]] * 1e6 / per[k] / comp[k] for k in comp}
    host = None if a.no_cpu else host_tls13_ladder_leg(alg, cipher, pl, sl, raw.tobytes(), traw.tobytes(), min(2048, n))
    cps = {k: n / (ms_[k + "_call"] / 1e3) for k in ("hs", "app")}

    def stage(k):
        return {"connections_per_s": round(cps[k]), "ms_per_batch_events": round(ms_[k + "_call"], 4),
                "ms_per_batch_wall": round(wall[k + "_call"] * 1e3, 4),
                "derive_kernel_ms": round(ms_[k + "_derive_kernel"], 4),
                "key_setup_ms": round(ms_[k + "_call"] - ms_[k + "_derive_kernel"], 4),
                "compressions_per_connection": comp[k],
                "derive_kernel_ns_per_compression": round(ns[k], 4),
                "per_compression_vs_tls12_kernel_same_hash": round(ns[k] / ns["tls12"], 3),
                "speedup_vs_host_path": round(cps[k] / host["handshake" if k == "hs" else "application"]["value"], 1)
                if host else None}
    print(json.dumps({
        "metric": "TLS 1.3 handshake-stage key derivations into the key table per second", "value": round(cps["hs"]),
        "unit": "connections/s", "count": n, "slots": 2 * n, "cipher": cipher, "hash": hname, "psk_len": pl,
        "shared_len": sl, "handshake_stage": stage("hs"), "application_stage": stage("app"),
        "batch_verify_data": {"count": 2 * n, "ms": round(ms_["verify_data"], 4),
                              "ns_per_compression": round(ns["verify_data"], 4)},
        "batch_derive_secret": {"count": n, "label": "res master", "ms": round(ms_["derive_secret"], 4),
                                "ns_per_compression": round(ns["derive_secret"], 4)},
        "tls12_aes128gcm_same_run": {"prf": hname, "derive_kernel_ms": round(ms_["tls12_derive_kernel"], 4),
                                     "compressions_per_connection": comp["tls12"],
                                     "derive_kernel_ns_per_compression": round(ns["tls12"], 4)},
        "host_path": host,
        "roofline": rowlib.roofline((176 + 5 * 48 + 128) * n, ms_["hs_call"], "per connection: the 176-byte "
                                    "tlsrec_tls13_hs_conn read, five 48-byte secrets and two 64-byte key records "
                                    "written; the key-table slots the key setup builds are not counted",
                                    "tls13 handshake stage + key setup")}))


def host_tls13_early_leg(hash_alg, cipher, psk_len, raw, sample, keys):
    """The path without the batch, for `sample` connections: the single-shot
    binder per connection and, with `keys`, the Early Secret, its two secrets
    and the key / iv (a synchronised job chain per step, every secret back on
    the host), then one tlsrec_keytab_load."""
    import torch
    import mbedtls_amd as M
    from mbedtls_amd import keysched as K
    H, kl = K.HASH_LEN[hash_alg], M.KEYLEN[cipher]
    kt = M.KeyTable(sample)
    K.evolve_secret(hash_alg, None, None)                        # the control-path stream and arena exist
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pairs = []
    for i in range(sample):
        c = raw[144 * i:144 * i + 144]
        K.create_psk_binder(hash_alg, c[:psk_len], K.PSK_RESUMPTION, c[48:48 + H])
        if keys:
            early = K.evolve_secret(hash_alg, None, c[:psk_len])
            ce, _ = K.derive_early_secrets(hash_alg, early, c[96:96 + H])
            ck, civ, _, _ = K.make_traffic_keys(hash_alg, ce, ce, kl, 12)
            pairs.append((ck, civ))
    ladder = time.perf_counter() - t0
    load = 0.0
    if keys:
        km = np.concatenate([M.key_material(cipher, M.VERSION_TLS1_3, k, iv) for k, iv in pairs])
        t0 = time.perf_counter()
        kt.load(km)
        torch.cuda.synchronize()
        load = time.perf_counter() - t0
    kt.close()
    return {"value": round(sample / (ladder + load)), "unit": "connections/s", "sample_connections": sample,
            "us_per_connection": round((ladder + load) / sample * 1e6, 2), "ladder_seconds": round(ladder, 4),
            "keytab_load_seconds": round(load, 4),
            "what": "per connection create_psk_binder" + (", evolve_secret (the Early Secret derive_early_secrets takes), "
                    "derive_early_secrets, make_traffic_keys, then one tlsrec_keytab_load of the records" if keys else "")
                    + "; wall time"}


def main_tls13_early(a):
    """tlsrec_tls13_keytab_derive_early (--no-keys: tlsrec_tls13_batch_psk_binder),
    its derive kernel alone, the binder-only kernel, tlsrec_tls13_batch_ticket_psk,
    the host path they replace, and the handshake-stage derive kernel of the same
    run under the same hash as the ns-per-compression yardstick."""
    from tools import rowlib
    import torch
    import mbedtls_amd as M
    from mbedtls_amd import keysched as K
    from mbedtls_amd.batch import _ptr, _stream
    from tests.prng import prng_array
    dev = torch.device("cuda")
    L = M.load()
    vp, u32, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    L.tlsrec__tls13_stage_hs_keys.restype = ci
    L.tlsrec__tls13_stage_hs_keys.argtypes = [vp, u32, u32, ci, u32, u32, vp, vp, vp, vp, vp]
    L.tlsrec__tls13_stage_early_keys.restype = ci
    L.tlsrec__tls13_stage_early_keys.argtypes = [vp, u32, u32, ci, u32, ci, vp, vp, vp, vp, vp, vp, vp]
    cipher, pl, n, keys = a.cipher, a.psk_len, a.count, not a.no_keys
    sha384 = cipher == M.CIPHER_AES_256_GCM
    hname, alg = ("sha384", K.ALG_SHA_384) if sha384 else ("sha256", K.ALG_SHA_256)
    raw = prng_array(0x7155, n * 144)
    conns = torch.from_numpy(raw).to(dev)
    hconns = torch.from_numpy(prng_array(0x7153, n * 176)).to(dev)
    nonces = torch.from_numpy(prng_array(0x7156, n * 32)).to(dev)

    def buf(k):
        return torch.zeros(k * 48, dtype=torch.uint8, device=dev)

    off, bd, ce, ex, rm, psk, hs, fin, ms = buf(n), buf(n), buf(n), buf(n), buf(n), buf(n), buf(2 * n), buf(2 * n), buf(n)
    rm.copy_(torch.from_numpy(prng_array(0x7157, n * 48)).to(dev))
    mt = torch.zeros(n, dtype=torch.int32, device=dev)
    kt, kths = M.KeyTable(n), M.KeyTable(2 * n)
    res = K.PSK_RESUMPTION
    sl = 48 if sha384 else 32

    def ok(r):
        assert r == 0, r

    s = _stream(None)
    K.batch_psk_binder(alg, pl, res, conns, None, off, None, n)      # the offered binders are the right ones
    legs = {
        "binder": lambda: K.batch_psk_binder(alg, pl, res, conns, off, bd, mt, n),
        "ticket_psk": lambda: K.batch_ticket_psk(alg, 32, rm, nonces, psk, n),
        "hs_derive_kernel": lambda: ok(L.tlsrec__tls13_stage_hs_keys(kths.handle, 0, n, cipher, pl, sl, _ptr(hconns),
                                                                      _ptr(hs), _ptr(fin), _ptr(ms), s)),
    }
    if keys:
        legs["early_derive_kernel"] = lambda: ok(L.tlsrec__tls13_stage_early_keys(
            kt.handle, 0, n, cipher, pl, res, _ptr(conns), _ptr(off), _ptr(bd), _ptr(mt), _ptr(ce), _ptr(ex), s))
        legs["early_call"] = lambda: K.keytab_derive_early(kt, 0, n, cipher, pl, res, conns, off, bd, mt, ce, ex)
    ms_, wall = {}, {}
    for name, fn in legs.items():
        fn()
        torch.cuda.synchronize()
        ms_[name], wall[name] = rowlib.event_timed(fn, a.steps)
    assert int(mt.sum().item()) == n
    comp = {"binder": 14, "ticket_psk": 4, "hs_derive_kernel": 8 + 2 + 2 + 4 + 6 + 16, "early_derive_kernel": 24}
    ns = {k: ms_[k] * 1e6 / n / comp[k] for k in comp if k in ms_}
    host = None if a.no_cpu else host_tls13_early_leg(alg, cipher, pl, raw.tobytes(), min(2048, n), keys)
    call = "early_call" if keys else "binder"
    kern = "early_derive_kernel" if keys else "binder"
    cps = n / (ms_[call] / 1e3)
    print(json.dumps({
        "metric": "TLS 1.3 PSK binder checks" + (" and 0-RTT key derivations into the key table" if keys else "") +
                  " per second", "value": round(cps), "unit": "connections/s", "count": n, "slots": n if keys else 0,
        "cipher": cipher, "hash": hname, "psk_len": pl, "keys": int(keys),
        "call": "tlsrec_tls13_keytab_derive_early" if keys else "tlsrec_tls13_batch_psk_binder",
        "ms_per_batch_events": round(ms_[call], 4), "ms_per_batch_wall": round(wall[call] * 1e3, 4),
        "derive_kernel_ms": round(ms_[kern], 4), "key_setup_ms": round(ms_[call] - ms_[kern], 4),
        "compressions_per_connection": comp[kern], "derive_kernel_ns_per_compression": round(ns[kern], 4),
        "per_compression_vs_hs_kernel_same_run": round(ns[kern] / ns["hs_derive_kernel"], 3),
        "binder_only": {"ms": round(ms_["binder"], 4), "compressions_per_connection": 14,
                        "ns_per_compression": round(ns["binder"], 4),
                        "per_compression_vs_hs_kernel_same_run": round(ns["binder"] / ns["hs_derive_kernel"], 3)},
        "batch_ticket_psk": {"count": n, "nonce_len": 32, "ms": round(ms_["ticket_psk"], 4),
                             "ns_per_compression": round(ns["ticket_psk"], 4)},
        "hs_kernel_same_run": {"psk_len": pl, "shared_len": sl, "derive_kernel_ms": round(ms_["hs_derive_kernel"], 4),
                               "compressions_per_connection": comp["hs_derive_kernel"],
                               "derive_kernel_ns_per_compression": round(ns["hs_derive_kernel"], 4)},
        "host_path": host, "speedup_vs_host_path": round(cps / host["value"], 1) if host else None,
        "roofline": rowlib.roofline((144 + 48 + 4 + (3 * 48 + 64 if keys else 48)) * n, ms_[call], "per connection: the "
                                    "144-byte tlsrec_tls13_psk_conn and the 48-byte offered binder read, the match "
                                    "word, the binder" + (", two 48-byte secrets and one 64-byte key record" if keys
                                                          else "") + " written; the key-table slots the key setup "
                                    "builds are not counted", "tls13 early stage" + (" + key setup" if keys else ""))}))


def master_compressions(hname, pms_len, ems):
    """SHA-2 compressions per connection of tls12_master_kernel"""
    if hname == "sha384":
        return 7
    return (12 if ems else 13) + (0 if pms_len <= 64 else 2 if pms_len <= 119 else 3)


def host_tls12_handshake_leg(prf, hname, pms_len, ems, raw, traw, n):
    """tlsrec_tls12_compute_master + tlsrec_tls12_calc_finished per connection: two synchronised round trips"""
    from mbedtls_amd import tls12 as T
    hl = 48 if hname == "sha384" else 32

    def one(i):
        c = raw[240 * i:240 * i + 240]
        m = T.tls12_compute_master(prf, c[:pms_len], c[192:192 + hl] if ems else c[128:192], ems)
        return T.tls12_calc_finished(prf, m, traw[48 * i:48 * i + hl], T.IS_CLIENT)

    one(0)
    t0 = time.perf_counter()
    for i in range(n):
        one(i)
    dt = time.perf_counter() - t0
    return {"value": round(n / dt), "unit": "connections/s", "kind": "single-shot", "leg": "host_path",
            "seconds": round(dt, 4),
            "sample": f"{n} connections: tlsrec_tls12_compute_master + tlsrec_tls12_calc_finished each; wall time"}


def main_tls12_handshake(a):
    """the two handshake batches, their chain into the key expansion, the host path they replace, and the
    key-expansion derive kernel of the same run under the same hash as the ns-per-compression yardstick"""
    from tools import rowlib
    import torch
    import mbedtls_amd as M
    from mbedtls_amd import tls12 as T
    from mbedtls_amd.batch import _ptr, _stream
    from tests.prng import prng_array
    dev = torch.device("cuda")
    L = M.load()
    vp, u32, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    L.tlsrec__tls12_stage_keys.restype = ci
    L.tlsrec__tls12_stage_keys.argtypes = [vp, u32, u32, ci, ci, vp, vp]
    hname, n, pl, ems = a.prf, a.count, a.pms_len, bool(a.ems)
    sha384 = hname == "sha384"
    prf = T.PRF_SHA384 if sha384 else T.PRF_SHA256
    cipher = M.CIPHER_AES_256_GCM if sha384 else M.CIPHER_AES_128_GCM
    raw = prng_array(0x7158, n * 240)
    traw = prng_array(0x7159, n * 48)
    conns = torch.from_numpy(raw).to(dev)
    trs = torch.from_numpy(traw).to(dev)
    out = torch.zeros(n * 112, dtype=torch.uint8, device=dev)
    off = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    vd = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    mt = torch.zeros(n, dtype=torch.int32, device=dev)
    kt, kty = M.KeyTable(2 * n), M.KeyTable(2 * n)

    def ok(r):
        assert r == 0, r

    def chain():
        T.tls12_batch_compute_master(prf, pl, ems, conns, out, n)
        T.tls12_keytab_derive(kt, 0, n, cipher, prf, out)

    s = _stream(None)
    T.tls12_batch_compute_master(prf, pl, ems, conns, out, n)
    T.tls12_batch_verify_data(prf, T.IS_CLIENT, out, trs, None, off, None, n)     # the offered values are the right ones
    legs = {
        "master": lambda: T.tls12_batch_compute_master(prf, pl, ems, conns, out, n),
        "chain": chain,
        "derive_call": lambda: T.tls12_keytab_derive(kt, 0, n, cipher, prf, out),
        "verify_data": lambda: T.tls12_batch_verify_data(prf, T.IS_CLIENT, out, trs, off, vd, mt, n),
        "stage_keys_aes128": lambda: ok(L.tlsrec__tls12_stage_keys(kty.handle, 0, n, M.CIPHER_AES_128_GCM, prf,
                                                                   _ptr(out), s)),
    }
    ms_, wall = {}, {}
    for name, fn in legs.items():
        fn()
        torch.cuda.synchronize()
        ms_[name], wall[name] = rowlib.event_timed(fn, a.steps)
    assert int(mt.sum().item()) == n
    # the AES-128-GCM key block is 40 bytes: 2 P_SHA256 iterations (5n + 3 = 13), 1 P_SHA384 iteration (5n + 2 = 7)
    comp = {"master": master_compressions(hname, pl, ems), "verify_data": 6 if sha384 else 7,
            "stage_keys_aes128": 7 if sha384 else 13}
    ns = {k: ms_[k] * 1e6 / n / comp[k] for k in comp}
    nh = min(2048, n)
    host = None if a.no_cpu else host_tls12_handshake_leg(prf, hname, pl, ems, raw.tobytes()[:240 * nh],
                                                          traw.tobytes()[:48 * nh], nh)
    cps = {k: n / (ms_[k] / 1e3) for k in ("master", "chain", "verify_data")}
    print(json.dumps({
        "metric": "TLS 1.2 master secrets derived per second", "value": round(cps["master"]), "unit": "connections/s",
        "count": n, "hash": hname, "pms_len": pl, "extended_ms": int(ems), "call": "tlsrec_tls12_batch_compute_master",
        "ms_per_batch_events": round(ms_["master"], 4), "ms_per_batch_wall": round(wall["master"] * 1e3, 4),
        "compressions_per_connection": comp["master"], "ns_per_compression": round(ns["master"], 4),
        "per_compression_vs_stage_keys_same_run": round(ns["master"] / ns["stage_keys_aes128"], 3),
        "chain": {"calls": "tlsrec_tls12_batch_compute_master -> tlsrec_tls12_keytab_derive", "cipher": cipher,
                  "slots": 2 * n, "connections_per_s": round(cps["chain"]), "ms": round(ms_["chain"], 4),
                  "ms_wall": round(wall["chain"] * 1e3, 4), "keytab_derive_alone_ms": round(ms_["derive_call"], 4)},
        "batch_verify_data": {"connections_per_s": round(cps["verify_data"]), "ms": round(ms_["verify_data"], 4),
                              "compressions_per_connection": comp["verify_data"],
                              "ns_per_compression": round(ns["verify_data"], 4),
                              "per_compression_vs_stage_keys_same_run":
                                  round(ns["verify_data"] / ns["stage_keys_aes128"], 3)},
        "stage_keys_same_run": {"cipher": M.CIPHER_AES_128_GCM, "derive_kernel_ms": round(ms_["stage_keys_aes128"], 4),
                                "compressions_per_connection": comp["stage_keys_aes128"],
                                "derive_kernel_ns_per_compression": round(ns["stage_keys_aes128"], 4)},
        "host_path": host, "speedup_vs_host_path": round(min(cps["master"], cps["verify_data"]) / host["value"], 1)
        if host else None,
        "roofline": rowlib.roofline((16 * ((pl + 15) // 16) + 64 + (48 if ems else 0) + 112) * n, ms_["master"],
                                    "per connection: the premaster's 16-byte groups, the 64 random bytes and with "
                                    "extended_ms the session hash read, the 112-byte tlsrec_tls12_conn written",
                                    "tls12 master secret")}))


EXPORTER_SHAPES = {
    # name: (label, shared context or None, bytes)
    "dtls_srtp": (b"EXTRACTOR-dtls_srtp", None, 60),                    # RFC 5764 4.2
    "eap_tls": (b"EXPORTER_EAP_TLS_Key_Material", b"\x0d", 128),        # RFC 9190 2.3: the one-byte type code
    "channel_binding": (b"EXPORTER-Channel-Binding", None, 32),         # RFC 9266
}


def exporter_compressions(version, hname, label_len, ctx_len, out_len):
    """SHA-2 compressions per connection of the exporter kernels (exporters); ctx_len None = no context"""
    H, bb, lenb = (48, 128, 16) if hname == "sha384" else (32, 64, 8)

    def b(nbytes):
        return (nbytes + 1 + lenb + bb - 1) // bb

    iters = (out_len + H - 1) // H
    if version == "tls13":
        return 2 + b(11 + label_len + H) + 1 + 2 + (b(ctx_len) if ctx_len else 0) + 2 + 3 * (iters - 1)
    n = label_len + 64 + (0 if ctx_len is None else 2 + ctx_len)
    return 2 + b(n) + 1 + iters * (b(H + n) + 1) + 2 * (iters - 1)


def main_exporter(a):
    """both exporter batches at the three deployment shapes, the host path each replaces (the single-shot call per
    connection on at most 2 048 connections) and the key-expansion derive kernel of the same run under the same hash
    as the ns-per-compression yardstick; one JSON line per (version, shape)"""
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
    hname, n = a.prf, a.count
    sha384 = hname == "sha384"
    H = 48 if sha384 else 32
    prf, alg = (T.PRF_SHA384, K.ALG_SHA_384) if sha384 else (T.PRF_SHA256, K.ALG_SHA_256)
    craw = prng_array(0x715A, n * 112)
    sraw = prng_array(0x715B, n * 48)
    conns = torch.from_numpy(craw).to(dev)
    secrets = torch.from_numpy(sraw).to(dev)
    kty = M.KeyTable(2 * n)
    s = _stream(None)

    def yard():
        r = L.tlsrec__tls12_stage_keys(kty.handle, 0, n, M.CIPHER_AES_128_GCM, prf, _ptr(conns), s)
        assert r == 0, r

    yard()
    torch.cuda.synchronize()
    yard_ms, _ = rowlib.event_timed(yard, a.steps)
    yard_comp = 7 if sha384 else 13
    yard_ns = yard_ms * 1e6 / n / yard_comp
    nh = min(2048, n)
    cb, sb = craw.tobytes(), sraw.tobytes()
    for version in ("tls13", "tls12"):
        for shape, (label, ctx, out_len) in EXPORTER_SHAPES.items():
            stride = (out_len + 15) & ~15
            out = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
            ctxs = None if ctx is None else torch.from_numpy(np.frombuffer(ctx, dtype=np.uint8).copy()).to(dev)
            cl = len(ctx) if ctx else 0
            if version == "tls13":
                name = "tlsrec_tls13_batch_exporter"

                def fn():
                    K.batch_exporter(alg, secrets, label, ctxs, cl, 0, out, out_len, stride, n)

                def one(i):
                    return K.exporter(alg, sb[48 * i:48 * i + H], label, ctx or b"", out_len)
            else:
                name = "tlsrec_tls12_batch_export_keying_material"

                def fn():
                    T.batch_export_keying_material(prf, conns, label, ctxs, cl, 0, ctx is not None, out, out_len, stride, n)

                def one(i):
                    c = cb[112 * i:112 * i + 112]
                    return T.tls12_export_keying_material(prf, c[:48], c[48:], label, ctx, out_len)
            fn()
            torch.cuda.synchronize()
            ms, wall = rowlib.event_timed(fn, a.steps)
            got = out.cpu().numpy().tobytes()
            host = None
            if not a.no_cpu:
                assert one(0) == got[:out_len]
                t0 = time.perf_counter()
                for i in range(nh):
                    one(i)
                dt = time.perf_counter() - t0
                assert one(nh - 1) == got[stride * (nh - 1):stride * (nh - 1) + out_len]
                host = {"value": round(nh / dt), "unit": "connections/s", "kind": "single-shot", "leg": "host_path",
                        "seconds": round(dt, 4), "sample": f"{nh} connections: the single-shot call each; wall time"}
            comp = exporter_compressions(version, hname, len(label), None if ctx is None else len(ctx), out_len)
            ns = ms * 1e6 / n / comp
            cps = n / (ms / 1e3)
            print(json.dumps({
                "metric": "keying material exported per second", "value": round(cps), "unit": "connections/s",
                "count": n, "version": version, "hash": hname, "shape": shape, "call": name,
                "label_len": len(label), "context_len": None if ctx is None else len(ctx), "out_len": out_len,
                "out_stride": stride, "ms_per_batch_events": round(ms, 4), "ms_per_batch_wall": round(wall * 1e3, 4),
                "compressions_per_connection": comp, "ns_per_compression": round(ns, 4),
                "per_compression_vs_stage_keys_same_run": round(ns / yard_ns, 3),
                "stage_keys_same_run": {"cipher": M.CIPHER_AES_128_GCM, "derive_kernel_ms": round(yard_ms, 4),
                                        "compressions_per_connection": yard_comp,
                                        "derive_kernel_ns_per_compression": round(yard_ns, 4)},
                "host_path": host, "speedup_vs_host_path": round(cps / host["value"], 1) if host else None,
                "roofline": rowlib.roofline(((48 if version == "tls13" else 112) + out_len) * n, ms,
                                            "per connection: the secret (48 bytes) or the tlsrec_tls12_conn (112) read, "
                                            "out_len bytes written", "exporter")}), flush=True)


# ---- X25519 -----------------------------------------------------------------------------------
def x25519_cpu_worker(seconds):
    """one process of the CPU leg: EVP_PKEY_derive over fresh key pairs for `seconds`; prints its count"""
    from tests import x25519_ref as R
    from tests.prng import prng_bytes
    if R.lib() is None:
        print(0)
        return
    L = R.lib()
    raw = prng_bytes(os.getpid(), 64)
    # one context for the process, set up outside the timed loop (making the private key object costs a
    # ladder of its own, which the reference pays in psa_generate_key, not in the agreement)
    key = L.EVP_PKEY_new_raw_private_key(R.EVP_PKEY_X25519, None, raw[:32], 32)
    peer = L.EVP_PKEY_new_raw_public_key(R.EVP_PKEY_X25519, None, R.model(raw[32:], R.BASE), 32)
    ctx = L.EVP_PKEY_CTX_new(key, None)
    assert L.EVP_PKEY_derive_init(ctx) == 1 and L.EVP_PKEY_derive_set_peer(ctx, peer) == 1
    out, ln = ctypes.create_string_buffer(32), ctypes.c_size_t(32)
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(64):
            assert L.EVP_PKEY_derive(ctx, out, ctypes.byref(ln)) == 1
        n += 64
    print(n / (time.perf_counter() - t0))


def x25519_cpu_leg(seconds):
    """EVP_PKEY_derive per second on min(16, CPUs) worker processes, none of which opens the GPU"""
    import subprocess
    workers = max(1, min(16, os.cpu_count() or 1, int(os.environ.get("OMP_NUM_THREADS", "16"))))
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--x25519-cpu-worker", "--cpu-seconds",
                               str(seconds)], stdout=subprocess.PIPE, text=True) for _ in range(workers)]
    rates = [float(p.communicate()[0].strip() or 0) for p in procs]
    return {"kind": "evp", "workers": workers, "derives_per_second": round(sum(rates)),
            "per_worker": round(sum(rates) / workers), "seconds": seconds,
            "note": "EVP_PKEY_derive alone, one context per worker process, through ctypes"}


def main_x25519(a):
    cpu = None if a.no_cpu else x25519_cpu_leg(a.cpu_seconds)      # before this process opens the GPU
    import torch
    import mbedtls_amd as M
    from mbedtls_amd import keysched as K, x25519 as XK
    from tests.prng import prng_array
    dev = torch.device("cuda")
    st = torch.cuda.current_stream()
    rep = "ten signed limbs of 25.5 bits, 64-bit products"

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
        for s, e in ev:
            s.record(st)
            fn()
            e.record(st)
        torch.cuda.synchronize()
        return [s.elapsed_time(e) for s, e in ev]

    def row(leg, count, ms, **extra):
        m = float(np.median(ms))
        r = {"metric": "X25519 per second", "leg": leg, "count": count, "value": round(count / (m / 1e3)),
             "unit": "connections/s", "ms_per_call_median": round(m, 4), "ms_per_call": [round(x, 4) for x in ms],
             "representation": rep}
        if cpu and cpu["derives_per_second"]:
            r["ratio_to_cpu"] = round(r["value"] / cpu["derives_per_second"], 2)
        r.update(extra)
        print(json.dumps(r), flush=True)
        return m

    if cpu:
        print(json.dumps({"metric": "X25519 per second", "leg": "cpu_evp_pkey_derive", **cpu}), flush=True)
    for count in (4096, 65536, 1048576):
        priv = torch.from_numpy(prng_array(0x255 + count, count * 32)).to(dev)
        pub = torch.zeros(count * 32, dtype=torch.uint8, device=dev)
        out = torch.zeros(count * 32, dtype=torch.uint8, device=dev)
        ok = torch.zeros(count, dtype=torch.int32, device=dev)
        row("batch_public", count, timed(lambda: XK.batch_public(priv, pub, count)))
        row("batch_shared", count, timed(lambda: XK.batch_shared(priv, pub, out, ok, count)))
        assert int(ok.sum()) == count
    # the chain: the shared secret lands in hs_conn.shared, the handshake stage follows on the stream
    count, cipher = a.count, M.CIPHER_AES_128_GCM
    priv = torch.from_numpy(prng_array(0x2551, count * 32)).to(dev)
    pub = torch.zeros(count * 32, dtype=torch.uint8, device=dev)
    XK.batch_public(priv, pub, count)
    conns = torch.from_numpy(prng_array(0x2552, count * K.HS_CONN_BYTES)).to(dev)
    ok = torch.zeros(count, dtype=torch.int32, device=dev)
    hs, ms_ = (torch.zeros(n * 48, dtype=torch.uint8, device=dev) for n in (2 * count, count))
    kt = M.KeyTable(2 * count)
    dst, stride = XK.into_hs_conns(conns)

    def stage():
        K.keytab_derive_handshake(kt, 0, count, cipher, 0, 32, conns, hs, None, ms_)

    def chain():
        XK.batch_shared(priv, pub, dst, ok, count, out_stride=stride)
        stage()

    t_stage = float(np.median(timed(stage)))
    t_x = float(np.median(timed(lambda: XK.batch_shared(priv, pub, dst, ok, count, out_stride=stride))))
    row("chain batch_shared -> tls13_keytab_derive_handshake", count, timed(chain),
        ms_handshake_stage_alone=round(t_stage, 4), ms_batch_shared_alone=round(t_x, 4),
        key_exchange_share_of_chain=round(t_x / (t_x + t_stage), 4))
    kt.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--x25519", action="store_true",
                    help="the key exchange batches (tlsrec_x25519_batch_public, _batch_shared) and their chain into "
                         "the TLS 1.3 handshake stage")
    ap.add_argument("--x25519-cpu-worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--exporter", action="store_true",
                    help="the exporter batches (tlsrec_tls13_batch_exporter, tlsrec_tls12_batch_export_keying_material) "
                         "at the DTLS-SRTP, EAP-TLS and channel-binding shapes under --prf")
    ap.add_argument("--tls12-handshake", action="store_true",
                    help="the TLS 1.2 handshake batches (tlsrec_tls12_batch_compute_master, _batch_verify_data)")
    ap.add_argument("--pms-len", type=int, default=32, help="--tls12-handshake: 1..128")
    ap.add_argument("--ems", action="store_true", help="--tls12-handshake: extended master secret (RFC 7627)")
    ap.add_argument("--tls13-early", action="store_true",
                    help="the resumed-handshake batches (tlsrec_tls13_keytab_derive_early, _batch_psk_binder, "
                         "_batch_ticket_psk)")
    ap.add_argument("--no-keys", action="store_true", help="--tls13-early: the binder alone, no table")
    ap.add_argument("--tls13-handshake", action="store_true",
                    help="the TLS 1.3 ladder batches (tlsrec_tls13_keytab_derive_handshake / _application)")
    ap.add_argument("--psk-len", type=int, default=32, help="--tls13-handshake: 0..48; --tls13-early: 1..48")
    ap.add_argument("--shared-len", type=int, default=32, help="--tls13-handshake: 0, 32, 48, 56 or 66")
    ap.add_argument("--count", type=int, default=65536)
    ap.add_argument("--cipher", type=int, default=None, help="default 2 (with --cbc-mac: the suite's, 23 or 24)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--update", type=int, default=1)
    ap.add_argument("--cpu-seconds", type=float, default=2.0, help="wall-time target of the CPU sample")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--tls12", action="store_true", help="the TLS 1.2 key expansion (tlsrec_tls12_keytab_derive)")
    ap.add_argument("--prf", choices=["sha256", "sha384"], default=None,
                    help="--tls12: the suite's PRF hash (default sha256; with --cbc-mac 3 sha384)")
    ap.add_argument("--cbc-mac", type=int, choices=[1, 2, 3], default=0,
                    help="--tls12: an AES-CBC + HMAC suite (1 SHA-1, 2 SHA-256, 3 SHA-384), tlsrec_tls12_keytab_derive_cbc")
    ap.add_argument("--etm", action="store_true", help="--cbc-mac: encrypt-then-MAC slots")
    a = ap.parse_args()
    if a.x25519_cpu_worker:
        return x25519_cpu_worker(a.cpu_seconds)
    if a.x25519:
        return main_x25519(a)
    if a.exporter:
        a.prf = a.prf or "sha256"
        return main_exporter(a)
    if a.tls12_handshake:
        a.prf = a.prf or "sha256"
        return main_tls12_handshake(a)
    if a.tls13_early:
        a.cipher = 1 if a.cipher is None else a.cipher
        return main_tls13_early(a)
    if a.tls13_handshake:
        a.cipher = 1 if a.cipher is None else a.cipher
        return main_tls13_handshake(a)
    if a.cbc_mac:
        if not a.tls12:
            ap.error("--cbc-mac goes with --tls12")
        return main_tls12_cbc(a)
    a.cipher = 2 if a.cipher is None else a.cipher
    a.prf = a.prf or "sha256"
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
