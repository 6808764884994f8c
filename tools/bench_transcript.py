#!/usr/bin/env python3
"""Transcript rows (profiles/r17/rows/transcript.jsonl).

    python tools/bench_transcript.py [--count 65536] [--steps 5] [--label shipped]

One JSON line per (hash, shape), tlsrec_transcript_batch_update over `count`
connections timed with HIP events on the call's stream (tools/rowlib.
event_timed: the fail-closed prefill and the kernel):

  clienthello_512   one 512-byte segment, RESET | SNAPSHOT
  flight_2k / _4k   four segments with four snapshots, every segment at an odd
                    arena offset
  flight_2k_aligned the same with every segment 16-byte aligned
  flight_2k_skewed  lengths uniform in 0.5 .. 4 KiB within each wave: what the
                    longest lane of a wave costs the others

Each row carries connections/s, GiB/s hashed, ns per compression (data blocks
and padding blocks), the same run's tlsrec_tls12_batch_verify_data under the
same hash (7 / 6 compressions per connection: the family's yardstick) and a
one-core hashlib loop over the same messages.  --label names the build:
TLSREC_LIBRARY pointing at a -DTLSREC_TRANSCRIPT_BYTEWISE variant
(tools/build_variant.sh) gives the byte-wise hot loop on the same box.
"""
from __future__ import annotations

import argparse
import hashlib
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
    ap.add_argument("--label", default="shipped")
    a = ap.parse_args()

    import torch
    import mbedtls_amd as M
    from mbedtls_amd import tls12 as T12
    from mbedtls_amd import transcript as T
    from tests.prng import prng_array
    from tools import rowlib

    dev = torch.device("cuda")
    n = a.count
    rng = np.random.default_rng(0x7115EC0DE)

    def shape(name):
        """per-connection segment lengths (n x nseg) and whether segments are 16-byte aligned"""
        if name == "clienthello_512":
            return np.full((n, 1), 512, np.int64), False
        if name == "flight_4k":
            return np.tile(np.array([1200, 1800, 300, 796], np.int64), (n, 1)), False
        if name == "flight_2k_skewed":
            total = rng.integers(512, 4097, size=n)
            return np.stack([total * 3 // 10, total * 4 // 10, total // 10,
                             total - total * 3 // 10 - total * 4 // 10 - total // 10], axis=1), False
        return np.tile(np.array([600, 900, 150, 398], np.int64), (n, 1)), name == "flight_2k_aligned"

    conns12 = torch.from_numpy(prng_array(0x7158, n * 112)).to(dev)
    trs12 = torch.from_numpy(prng_array(0x7159, n * 48)).to(dev)
    vd = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    for alg, hname, bb, lenb, prf, ycomp in ((M.ALG_SHA_256, "sha256", 64, 8, T12.PRF_SHA256, 7),
                                            (M.ALG_SHA_384, "sha384", 128, 16, T12.PRF_SHA384, 6)):
        yard = lambda: T12.tls12_batch_verify_data(prf, T12.IS_CLIENT, conns12, trs12, None, vd, None, n)  # noqa: E731
        yard()
        torch.cuda.synchronize()
        y_ms, _ = rowlib.event_timed(yard, a.steps)
        y_ns = y_ms * 1e6 / n / ycomp
        for name in ("clienthello_512", "flight_2k", "flight_4k", "flight_2k_aligned", "flight_2k_skewed"):
            lens, aligned = shape(name)
            nseg = lens.shape[1]
            # aligned: every segment on a 16-byte boundary; else an even pitch from offset 1: every offset odd
            flat = ((lens + 15) // 16 * 16 if aligned else (lens + 2) // 2 * 2).reshape(-1)
            offs = np.concatenate([[0], np.cumsum(flat)[:-1]]) + (0 if aligned else 1)
            assert (offs % 16 == 0).all() if aligned else (offs % 2 == 1).all()
            arena_len = int(offs[-1] + lens.reshape(-1)[-1]) + 16
            arena = torch.from_numpy(prng_array(0x7A5C, arena_len)).to(dev)
            segs = np.zeros(n * nseg, dtype=T.SEG)
            segs["off"], segs["len"] = offs, lens.reshape(-1)
            segs["out_off"] = np.arange(n * nseg, dtype=np.uint64) * 48
            segs["flags"] = T.SNAPSHOT
            segs["flags"][0::nseg] |= T.RESET
            conns = np.zeros(n, dtype=T.CONN)
            conns["state"] = np.arange(n)
            conns["first_seg"], conns["nseg"] = np.arange(n) * nseg, nseg
            d_segs = torch.from_numpy(segs.view(np.uint8).reshape(-1).copy()).to(dev)
            d_conns = torch.from_numpy(conns.view(np.uint8).reshape(-1).copy()).to(dev)
            states, status = T.new_states(n, dev), torch.zeros(n, dtype=torch.int32, device=dev)
            out = torch.zeros(n * nseg * 48, dtype=torch.uint8, device=dev)
            fn = lambda: T.batch_update(alg, states, d_conns, d_segs, arena, out, status)  # noqa: E731
            fn()
            torch.cuda.synchronize()
            ms, wall = rowlib.event_timed(fn, a.steps)
            assert int(status.abs().sum().item()) == 0
            # spot check and the host path: hashlib over the same messages on one core
            host = arena.cpu().numpy()
            m = min(n, 2048)
            t0 = time.perf_counter()
            for i in range(m):
                h = hashlib.new(hname)
                for k in range(nseg):
                    o = int(offs[i * nseg + k])
                    h.update(host[o:o + int(lens[i, k])])
                    d = h.digest()
            cpu = m / (time.perf_counter() - t0)
            got = out.cpu().numpy().reshape(n * nseg, 48)
            assert got[m * nseg - 1, :len(d)].tobytes() == d
            # compressions: data blocks plus, per snapshot, one or two padding blocks
            cum = np.cumsum(lens, axis=1)
            comp = int((cum[:, -1] // bb).sum() + (1 + (cum % bb >= bb - lenb)).sum())
            nbytes = int(lens.sum())
            ns = ms * 1e6 / comp
            # the wave runs as long as its longest lane: compressions the waves actually step through
            per_conn = cum[:, -1] // bb + (1 + (cum % bb >= bb - lenb)).sum(axis=1)
            pad = (-n) % 64
            wave_comp = int(np.pad(per_conn, (0, pad)).reshape(-1, 64).max(axis=1).sum() * 64)
            print(json.dumps({
                "row": f"transcript_{hname}_{name}", "label": a.label, "library": os.environ.get("TLSREC_LIBRARY", ""),
                "metric": "connections' transcripts advanced per second", "value": round(n / (ms / 1e3)),
                "unit": "connections/s", "count": n, "steps": a.steps, "segments": nseg,
                "bytes_per_connection_mean": round(nbytes / n, 1), "gib_per_s": round(nbytes / (ms / 1e3) / 2 ** 30, 2),
                "ms_per_batch_events": round(ms, 4), "ms_per_batch_wall": round(wall * 1e3, 4),
                "compressions": comp, "ns_per_compression": round(ns, 4),
                "lane_slots_stepped_over_compressions": round(wave_comp / comp, 3),
                "yardstick_same_run": {"call": "tlsrec_tls12_batch_verify_data", "prf": hname, "ms": round(y_ms, 4),
                                       "compressions_per_connection": ycomp, "ns_per_compression": round(y_ns, 4)},
                "per_compression_vs_verify_data_same_run": round(ns / y_ns, 3),
                "cpu_hashlib_one_core_connections_per_s": round(cpu),
                "cpu_note": "python hashlib loop over the same segments on one core, interpreter overhead included",
                "timing": "HIP events on the call's stream around each timed call (prefill and kernel)"}), flush=True)


if __name__ == "__main__":
    main()
