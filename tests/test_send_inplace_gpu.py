"""The in-place send path (the default of tlsrec_stream_encrypt /
tlsrec_dtls_encrypt for tables of AES-GCM and ChaCha20-Poly1305 keys without
CIDs: out_frame_conn_kernel<TlsWire / DtlsWire>, then the AEAD kernels read
each record's content at in + src_off[i]) against the oracle, byte for byte;
both calls are send_impl<W> over one set of kernels: record edges and odd
input offsets, few connections of many records, and every launch shape the
engine picks with src_off set.  Each test asserts its path from the
dispatchers' launch log; shapes are sized from the device's CU count by the
rules of batch.hip batch()."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

import mbedtls_amd as M  # noqa: E402
from mbedtls_amd import _abi  # noqa: E402
import oracle as O  # noqa: E402
from tests import batchlib as B  # noqa: E402
from tests.batchlib import launch_log  # noqa: E402,F401  (fixture)
from tests.prng import prng_array, prng_bytes  # noqa: E402,F401

CU = torch.cuda.get_device_properties(0).multi_processor_count
SRC_CIPHERS = [M.CIPHER_AES_128_GCM, M.CIPHER_AES_192_GCM, M.CIPHER_AES_256_GCM, M.CIPHER_CHACHA20_POLY1305]


def _bulk(seed, n):
    return prng_array(seed, n).tobytes()


def dctr(epoch, seq):
    return epoch.to_bytes(2, "big") + (seq % (1 << 48)).to_bytes(6, "big")


def _stream_slots(seed, ciphers, versions, count):
    return B.random_slots(seed, ciphers, versions, count)


def _dtls_slots(seed, ciphers, count):
    out = []
    for i in range(count):
        c = ciphers[i % len(ciphers)]
        b = prng_bytes(seed * 1000 + i, 48)
        out.append((c, b[:M.KEYLEN[c]], b[32:48], b""))
    return out


def _check_stream(c, jobs, got):
    for i, ((slot, pt, ctr, frag, typ), (r, out)) in enumerate(zip(jobs, got)):
        st, want, nrec, ctr2 = O.stream_encrypt(c.ot[slot], pt, typ, ctr.to_bytes(8, "big"), frag or 16384)
        assert (int(r["status"]), int(r["nrec"]), bytes(r["out_ctr"])) == (st, nrec, ctr2), i
        assert out == want, (i, slot, len(pt), frag)
        region = c.last_regions[i]
        assert region[len(out):] == bytes(len(region) - len(out)), (i, "bytes past out_len")


def _check_dtls(tab, jobs, got):
    for i, ((slot, pt, c8, frag, typ), (r, out, _, _)) in enumerate(zip(jobs, got)):
        st, want, nrec, c2 = O.dtls_encrypt(tab.ot[slot], pt, typ, c8, frag or 16384)
        assert (int(r["status"]), int(r["nrec"]), bytes(r["out_ctr"])) == (st, nrec, c2), i
        assert out == want, (i, slot, len(pt), frag)
        region = tab.last_regions[i]
        assert region[len(out):] == bytes(len(region) - len(out)), (i, "bytes past out_len")


def _assert_in_place(log, dtls, in_place=True):
    """the send frame of the call, and src_off on every AEAD launch"""
    assert log(_abi.LOG_SEND_FRAME) == [(_abi.LOG_SEND_FRAME, int(in_place), int(dtls), 0, 0)], log()
    aead = log(_abi.LOG_GCM) + log(_abi.LOG_CHACHA)
    assert aead and not log(_abi.LOG_ALT_GCM) and not log(_abi.LOG_CCM)
    assert all(e[4] == int(in_place) for e in log(_abi.LOG_GCM)), log()
    assert all(e[2] == int(in_place) for e in log(_abi.LOG_CHACHA)), log()


def _assert_copy_frame(log, dtls):
    """the send frame of a call whose table holds a CCM key or a CID: map + copy"""
    assert log(_abi.LOG_SEND_FRAME) == [(_abi.LOG_SEND_FRAME, 0, int(dtls), 0, 0)], log()


# ---- 1. edges ---------------------------------------------------------------------
def _edge_jobs():
    """(in_len, max_frag) for 64 jobs: every length kind at every fragment size"""
    combos = []
    for frag in (16, 100, 1400, 4096):
        combos += [(n, frag) for n in (0, 1, 15, 16, 17, frag - 1, frag, frag + 1, 16 * frag, 16 * frag + 1,
                                       17 * frag + 15, 40 * frag + 3)]
    combos += [(n, 0) for n in (0, 1, 15, 16, 17)]                  # max_frag 0 (16 384) with short inputs
    combos += [(17 * f + 15, f) for f in (16, 100, 1400)] + [(f + 1, f) for f in (16, 100, 1400, 4096)] + \
        [(15, 0), (17, 0), (40 * 16 + 3, 16), (40 * 100 + 3, 100)]
    assert len(combos) == 64
    return combos


def test_edges_stream(launch_log):
    slots = _stream_slots(301, SRC_CIPHERS, [M.VERSION_TLS1_2, M.VERSION_TLS1_3], 8)
    assert {(s[0], s[1]) for s in slots} == {(c, v) for c in SRC_CIPHERS for v in (M.VERSION_TLS1_2, M.VERSION_TLS1_3)}
    c = B.Conns(slots)
    jobs = []
    for i, (n, frag) in enumerate(_edge_jobs()):
        slot = (i + i // 8) % 8              # each length kind meets several ciphers / versions
        jobs.append((slot, _bulk(31000 + i, n), 0xA1B2C3D4E5F60718 + 0x0101010101010101 * (i % 5), frag,
                     22 if i % 3 == 0 else 23))
    launch_log.reset()
    got = c.encrypt(jobs, odd=True)
    _assert_in_place(launch_log, dtls=False)
    _check_stream(c, jobs, got)
    # ... and back through the receive path
    conns = [(slot, out, ctr, 0) for (slot, _, ctr, _, _), (_, out) in zip(jobs, got)]
    a, recs, res, sres, offs = c.decrypt(conns)
    for i, (slot, data, ctr, nbz) in enumerate(conns):
        want, wrecs, wbuf = O.stream_decrypt(c.ot[slot], data, ctr.to_bytes(8, "big"), nbz)
        g = sres[i]
        assert (int(g["status"]), int(g["nrec"]), int(g["consumed"]), bytes(g["in_ctr"]), int(g["nb_zero"])) == \
            (want["status"], want["nrec"], want["consumed"], want["in_ctr"], want["nb_zero"]), i
        f, pt, got_pt = int(g["first"]), jobs[i][1], b""
        for k, (off, doff, dlen, typ) in enumerate(wrecs):
            rr = res[f + k]
            assert (int(rr["data_offset"]), int(rr["data_len"]), int(rr["type"])) == (doff, dlen, typ)
            s0 = offs[i] + off + doff
            assert a[s0:s0 + dlen].tobytes() == wbuf[off + doff:off + doff + dlen]
            got_pt += a[s0:s0 + dlen].tobytes()
        if want["status"] == 0:
            assert got_pt == pt, i
    c.close()


def test_edges_dtls(launch_log):
    slots = _dtls_slots(302, SRC_CIPHERS, 8)
    tab = B.Table(slots)
    jobs = []
    for i, (n, frag) in enumerate(_edge_jobs()):
        slot = (i + i // 8) % 8
        jobs.append((slot, _bulk(32000 + i, n), dctr(0x0102 + 0x0101 * (i % 7), 0xA1B2C3D4E5F6 - 77 * i), frag,
                     22 if i % 3 == 0 else 23))
    launch_log.reset()
    got = tab.encrypt(jobs, odd=True)
    _assert_in_place(launch_log, dtls=True)
    _check_dtls(tab, jobs, got)
    # ... and back through the receive path, one record per datagram
    conns = []
    for (slot, pt, c8, frag, typ), (r, out, rc, rs) in zip(jobs, got):
        f, nrec = int(r["first"]), int(r["nrec"])
        starts = [int(rc[f + k]["buf_off"]) - 13 for k in range(nrec)]
        lens = [13 + int(rs[f + k]["data_len"]) for k in range(nrec)]
        base = starts[0] if starts else 0
        grams = [out[s - base:s - base + L] for s, L in zip(starts, lens)]
        assert b"".join(grams) == out
        conns.append((slot, {"in_epoch": int.from_bytes(c8[:2], "big")}, grams))
    B.check_vs_oracle(tab, conns, tab.decrypt(conns))
    tab.close()


# ---- 2. few connections, many records -----------------------------------------------
MANY = {"one-4096": [4096], "three-1000-17-1": [1000, 17, 1]}


@pytest.mark.parametrize("src", ["default", "0"], ids=["in-place", "copy"])
@pytest.mark.parametrize("dtls", [False, True], ids=["stream", "dtls"])
@pytest.mark.parametrize("shape", list(MANY), ids=list(MANY))
def test_few_connections_many_records(shape, dtls, src, monkeypatch, launch_log):
    """One connection of 4 096 records of 16 B, and three of 1 000 / 17 / 1 in
    one call (the last workgroup of the frame kernel partial, lane groups
    idle), read in place and (TLSREC_STREAM_SRC=0) copied first."""
    if src == "0":
        monkeypatch.setenv("TLSREC_STREAM_SRC", "0")
    else:
        monkeypatch.delenv("TLSREC_STREAM_SRC", raising=False)
    counts = MANY[shape]
    ciphers = [M.CIPHER_AES_256_GCM, M.CIPHER_CHACHA20_POLY1305, M.CIPHER_AES_192_GCM][:len(counts)]
    lens = [16 * n - (5 if n > 1 else 3) for n in counts]          # the last record short
    if dtls:
        tab = B.Table(_dtls_slots(303, ciphers, len(counts)))
        jobs = [(i, _bulk(33000 + i, n), dctr(3, 1000 * i + 5), 16, 23) for i, n in enumerate(lens)]
        launch_log.reset()
        got = tab.encrypt(jobs, odd=True)
        _assert_in_place(launch_log, dtls=True, in_place=src != "0")
        assert [int(g[0]["nrec"]) for g in got] == counts
        _check_dtls(tab, jobs, got)
        tab.close()
    else:
        c = B.Conns(_stream_slots(304, ciphers, [M.VERSION_TLS1_2, M.VERSION_TLS1_3][:len(counts)], len(counts)))
        jobs = [(i, _bulk(34000 + i, n), (1 << 40) + i, 16, 23) for i, n in enumerate(lens)]
        launch_log.reset()
        got = c.encrypt(jobs, odd=True)
        _assert_in_place(launch_log, dtls=False, in_place=src != "0")
        assert [int(g[0]["nrec"]) for g in got] == counts
        _check_stream(c, jobs, got)
        c.close()


# ---- 3. launch shapes with src_off --------------------------------------------------
# The rules of tlsrec_plan.h gcm_plan() / chacha_plan() for a grouped batch with a record-size hint
# (n records, nkeys loaded keys, rpk = n / nkeys, cu compute units):
#   one key           8 lanes, 16 waves, once n >= cu * 16 * 8 (Lfill); 4 lanes once
#                     n >= cu * 16 * 16 and the records are <= 4 KiB
#   rpk < 12          wave passes (-8): 16 lanes if rpk >= 3 and n >= cu * 16 * 2, else 64
#   paired (-32)      small records, 12 <= rpk < 256: Lp by tlsrec__gcm_pair_small_l
#                     (8 at 16, 4 at 32, 2 at 64 per key); records > 4 KiB: 32 lanes
#                     at 4..7 per key, 16 at 8..39; once n >= cu * 16 * (64 / Lp)
#   AES-192           none of the wave passes: 16-wave key passes, 8 lanes from 128
#                     records per key, 16 from 48, else 64 (and at least Lfill)
#   ChaCha            2 lanes from n >= cu * 8 * 32, 4 from cu * 8 * 16, else 8
# Each case sits at its threshold: the record count is the smallest the rule
# allows, so a case's bytes are count x record size -- 1.5 to 13 MB for the
# small-record cases; the two paired-big cases need records above 4 KiB
# (4 100 B here), which makes them 34 and 67 MB at 256 CUs, the oracle leg
# included 0.4 and 0.7 s as measured.
# tm (GcmArgs::tm with the environment's defaults, gcm_tm()): 1 for key
# passes, 9 for wave passes, 31 for the paired passes.
def _shape_cases(cu):
    G128, G192, G256, CH = SRC_CIPHERS
    return {
        # id: (cipher, nkeys, connections per key, records per connection, frag, dtls, expected log entry)
        "gcm-one-key-8": (G128, 1, 64, cu * 2, 48, False, (_abi.LOG_GCM, 8, 16, 1, 1)),
        "gcm-one-key-4": (G256, 1, 64, cu * 4, 48, False, (_abi.LOG_GCM, 4, 16, 1, 1)),
        "gcm-wave-16": (G256, cu * 8, 1, 4, 200, True, (_abi.LOG_GCM, 16, -8, 9, 1)),
        "gcm-wave-64": (G128, 48, 1, 2, 300, False, (_abi.LOG_GCM, 64, -8, 9, 1)),
        "gcm-pair-8": (G256, cu * 8, 1, 16, 100, True, (_abi.LOG_GCM, 8, -32, 31, 1)),
        "gcm-pair-4": (G128, cu * 8, 1, 32, 100, False, (_abi.LOG_GCM, 4, -32, 31, 1)),
        "gcm-pair-2": (G256, cu * 8, 1, 64, 100, False, (_abi.LOG_GCM, 2, -32, 31, 1)),
        "gcm-pair-big-32": (G128, cu * 8, 1, 4, 4100, False, (_abi.LOG_GCM, 32, -32, 31, 1)),
        "gcm-pair-big-16": (G256, cu * 4, 1, 16, 4100, False, (_abi.LOG_GCM, 16, -32, 31, 1)),
        # AES-192 has no wave-pass kernels (nr != 12 in batch()): 16-wave key passes, 64 lanes below 48
        # records per key, 16 from 48
        "gcm192-key-pass-64": (G192, cu * 8, 1, 4, 200, True, (_abi.LOG_GCM, 64, 16, 1, 1)),
        "gcm192-key-pass-16": (G192, cu * 8, 1, 64, 100, False, (_abi.LOG_GCM, 16, 16, 1, 1)),
        "chacha-8": (CH, 64, 1, cu, 64, False, (_abi.LOG_CHACHA, 8, 1)),
        "chacha-4": (CH, 64, 1, cu * 2, 64, True, (_abi.LOG_CHACHA, 4, 1)),
        "chacha-2": (CH, 64, 1, cu * 4, 64, False, (_abi.LOG_CHACHA, 2, 1)),
    }


SHAPE_IDS = list(_shape_cases(CU))


@pytest.mark.parametrize("case", SHAPE_IDS)
def test_launch_shape_with_src_off(case, monkeypatch, launch_log):
    for v in ("TLSREC_GCM_TREEMUL", "TLSREC_GCM_HBUILD", "TLSREC_GCM_WP", "TLSREC_GCM_PAIR", "TLSREC_GCM_PAIR_L",
              "TLSREC_GCM_LANES", "TLSREC_GROUPED", "TLSREC_STREAM_SRC"):
        monkeypatch.delenv(v, raising=False)            # the engine's defaults
    cipher, nkeys, cpk, rpc, frag, dtls, want = _shape_cases(CU)[case]
    n = nkeys * cpk * rpc
    # the thresholds the case was sized to (engine.hip), restated on this device's CU count
    if want[0] == _abi.LOG_CHACHA:
        rpwave = n // (CU * 8)
        assert want[1] == (2 if rpwave >= 32 else 4 if rpwave >= 16 else 8)
    elif want[2] == -32:
        assert n >= CU * 16 * (64 // want[1]) and nkeys > 1 and cipher != M.CIPHER_AES_192_GCM
    elif cipher == M.CIPHER_AES_192_GCM:
        rpk, rpwave = n // nkeys, n // (CU * 16)
        lfill = 8 if rpwave >= 8 else 16 if rpwave >= 2 else 64
        assert nkeys > 1 and want[1] == max(8 if rpk >= 128 else 16 if rpk >= 48 else 64, lfill)
    elif nkeys == 1:
        assert n // (CU * 16) >= (16 if want[1] == 4 else 8) and (want[1] == 4 or n // (CU * 16) < 16)
    else:
        assert n // nkeys < 12 and (want[1] == 64 or n // (CU * 16) >= 2)
    tails = min(frag, 97) if frag <= 4096 else 13      # (the paired-big cases: the mean stays above 4 096)
    version = M.VERSION_TLS1_2 if (dtls or len(case) % 2) else M.VERSION_TLS1_3
    if dtls:
        h = B.Table(_dtls_slots(305, [cipher], nkeys))
        jobs = [(i % nkeys, _bulk(35000 + i, rpc * frag - i % tails), dctr(1 + i % 3, 7 * i), frag, 23)
                for i in range(nkeys * cpk)]
    else:
        h = B.Conns(_stream_slots(306, [cipher], [version], nkeys))
        jobs = [(i % nkeys, _bulk(36000 + i, rpc * frag - i % tails), 11 * i, frag, 23)
                for i in range(nkeys * cpk)]
    if want[0] == _abi.LOG_GCM and want[2] == -32:      # the size hint the paired rule reads: small, or above 4 KiB
        assert frag <= 300 or sum(len(j[1]) for j in jobs) // n > 4096
    launch_log.reset()
    got = h.encrypt(jobs, odd=True)
    _assert_in_place(launch_log, dtls=dtls)
    entries = launch_log(want[0])
    if want[0] == _abi.LOG_GCM:
        assert entries == [want], entries
    else:
        assert [(e[0], e[1], e[2]) for e in entries] == [want], entries
    assert sum(int(g[0]["nrec"]) for g in got) == n
    (_check_dtls if dtls else _check_stream)(h, jobs, got)
    h.close()


# ---- 4. out_len against the size functions -------------------------------------------
def test_out_len_matches_out_size(launch_log):
    """The kernels' protected-length arithmetic and tlsrec_stream_out_size /
    tlsrec_dtls_out_size are one function per wire format: every connection's
    out_len equals out_size() for its slot and input length, and the length
    of the oracle's output.  Slots of granularity 0 / 16 / 64 over AES-128-GCM,
    AES-256-GCM, ChaCha20-Poly1305 and one CCM_8 slot; the stream run mixes
    TLS 1.2 and 1.3, the DTLS run slots without a CID and with a 3-byte one.
    A CCM key or a CID in the table means the copy path."""
    from mbedtls_amd import dtls as D
    from mbedtls_amd import stream as S
    G128, G256, CH, CCM8 = M.CIPHER_AES_128_GCM, M.CIPHER_AES_256_GCM, M.CIPHER_CHACHA20_POLY1305, \
        M.CIPHER_AES_128_CCM_8
    T12, T13 = M.VERSION_TLS1_2, M.VERSION_TLS1_3
    shape = [(G128, T12, 0), (G256, T13, 16), (CH, T13, 64), (CCM8, T12, 0),
             (G128, T13, 64), (G256, T12, 16), (CH, T12, 0), (G256, T13, 0)]
    keys = [prng_bytes(307000 + s, 48) for s in range(8)]
    edge = _edge_jobs()

    c = B.Conns([(ci, v, k[:M.KEYLEN[ci]], k[32:48], g) for (ci, v, g), k in zip(shape, keys)])
    jobs = [((i + i // 8) % 8, _bulk(37000 + i, n), 0x0102030405060708 + i, frag, 23) for i, (n, frag) in enumerate(edge)]
    launch_log.reset()
    got = c.encrypt(jobs, odd=True)
    _assert_copy_frame(launch_log, dtls=False)
    for i, ((slot, pt, ctr, frag, typ), (r, out)) in enumerate(zip(jobs, got)):
        ci, v, g = shape[slot]
        st, want, _, _ = O.stream_encrypt(c.ot[slot], pt, typ, ctr.to_bytes(8, "big"), frag or 16384)
        assert st == 0 and int(r["status"]) == 0, i
        assert int(r["out_len"]) == S.out_size(v, ci, g, len(pt), frag) == len(want), (i, slot, len(pt), frag)
    c.close()

    cids = [b"" if s % 2 == 0 else bytes([0xC0 + s, 1, 2]) for s in range(8)]
    tab = B.Table([(ci, k[:M.KEYLEN[ci]], k[32:48], cid) for (ci, _, _), k, cid in zip(shape, keys, cids)],
                  gran_of={s: g for s, (_, _, g) in enumerate(shape)})
    jobs = [((i + i // 8) % 8, _bulk(38000 + i, n), dctr(2 + i % 3, 1000 + 13 * i), frag, 23)
            for i, (n, frag) in enumerate(edge)]
    launch_log.reset()
    got = tab.encrypt(jobs, odd=True)
    _assert_copy_frame(launch_log, dtls=True)
    for i, ((slot, pt, c8, frag, typ), (r, out, _, _)) in enumerate(zip(jobs, got)):
        ci, _, g = shape[slot]
        st, want, _, _ = O.dtls_encrypt(tab.ot[slot], pt, typ, c8, frag or 16384)
        assert st == 0 and int(r["status"]) == 0, i
        assert int(r["out_len"]) == D.out_size(ci, g, len(cids[slot]), len(pt), frag) == len(want), \
            (i, slot, len(pt), frag)
    tab.close()
