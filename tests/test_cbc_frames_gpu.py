"""AES-CBC + HMAC connections through the stream and DTLS layers on the GPU
(tlsrec_stream_*_ex / tlsrec_dtls_*_ex with TLSREC_FRAME_CBC) against the
framing model of tests/cbc_frames_ref.py over the CBC record model of
tests/cbc_ref.py: byte-exact record streams and datagrams, descriptors,
per-connection results and every stop condition, with AEAD connections mixed
into the same calls (their results: the plain call's), under every receive
framing path the AEAD tests run, and the launch log's word that the framed
call reached the CBC kernel in identity order."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

import mbedtls_amd as M  # noqa: E402
from mbedtls_amd import _abi  # noqa: E402
from mbedtls_amd import dtls as D  # noqa: E402
from mbedtls_amd import stream as S  # noqa: E402
import oracle as O  # noqa: E402
from tests import batchlib as B  # noqa: E402
from tests import cbc_frames_ref as F  # noqa: E402
from tests import cbc_ref as R  # noqa: E402
from tests import cbclib as CL  # noqa: E402
from tests.batchlib import launch_log  # noqa: E402,F401  (fixture)
from tests.prng import prng_bytes  # noqa: E402

DEV = torch.device("cuda")
CANARY = 0xA5
A128, A256 = R.CIPHER_AES_128_CBC, R.CIPHER_AES_256_CBC

# the matrix: AES-128 / SHA-1 MAC-then-encrypt, AES-128 / SHA-256 encrypt-then-MAC, AES-256 / SHA-384
# MAC-then-encrypt; an AES-128-GCM TLS 1.2 and a ChaCha20-Poly1305 TLS 1.3 connection; an unloaded slot
STREAM_SLOTS = [CL.make_key(11, A128, R.MAC_SHA1, 0), CL.make_key(12, A128, R.MAC_SHA256, 1),
                CL.make_key(13, A256, R.MAC_SHA384, 0),
                (M.CIPHER_AES_128_GCM, M.VERSION_TLS1_2, prng_bytes(14, 16), prng_bytes(15, 12), 0),
                (M.CIPHER_CHACHA20_POLY1305, M.VERSION_TLS1_3, prng_bytes(16, 32), prng_bytes(17, 12), 0), None]
# DTLS: the same without and with connection IDs (slot 3: slot 1's key without its CID, slot 6: with another
# CID), AES-128-GCM and ChaCha20-Poly1305 under TLS 1.2
CID3, CID5 = b"\xaa\xbb\xcc", b"\x01\x02\x03\x04\x05"
DTLS_SLOTS = [CL.make_key(21, A128, R.MAC_SHA1, 0), CL.make_key(22, A128, R.MAC_SHA256, 1, CID3),
              CL.make_key(23, A256, R.MAC_SHA384, 0, CID5), CL.make_key(22, A128, R.MAC_SHA256, 1),
              (M.CIPHER_AES_128_GCM, M.VERSION_TLS1_2, prng_bytes(24, 16), prng_bytes(25, 12), 0),
              (M.CIPHER_CHACHA20_POLY1305, M.VERSION_TLS1_2, prng_bytes(26, 32), prng_bytes(27, 12), 0),
              CL.make_key(22, A128, R.MAC_SHA256, 1, b"\xaa\xbb\xcd")]


def ctr(epoch, seq):
    return epoch.to_bytes(2, "big") + (seq % (1 << 48)).to_bytes(6, "big")


def _al(x, a=128):
    return (x + a - 1) // a * a


def protector(slot, ivs=None):
    """the model's side of a slot (None: unloaded)"""
    if slot is None:
        return None
    if isinstance(slot, R.Key):
        return F.CbcProtector(slot, ivs or (lambda k: prng_bytes(77000 + k, 16)))
    c, v, k, iv, g = slot
    t = O.Transform(v, c, k, k, iv, iv, granularity=g or 16)
    return F.OracleAead(t, 8 if (v == M.VERSION_TLS1_2 and c != M.CIPHER_CHACHA20_POLY1305) else 0)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


# ---- send -------------------------------------------------------------------------
def send(kt, slots, jobs, dtls, cbc=True, ivs_arg="own"):
    """jobs: (slot, plaintext, out_ctr bytes, max_frag, type).  One call; returns the raw results."""
    ps = [protector(slots[j[0]]) for j in jobs]
    usable = [p is not None and not (dtls and p.tls13) for p in ps]
    counts = [(len(j[1]) + (j[3] or 16384) - 1) // (j[3] or 16384) if u else 0 for j, u in zip(jobs, usable)]
    firsts = [sum(counts[:i]) for i in range(len(jobs))]
    nmax = sum(counts) + 1
    ivs = prng_bytes(4242, 16 * nmax)
    sizes = [F.out_size(p, len(j[1]), j[3], dtls) if u else 0 for p, j, u in zip(ps, jobs, usable)]
    d = np.zeros(len(jobs), dtype=S.STREAM_OUT)
    pos_in, pos_out, outs = 0, 0, []
    for i, (slot, pt, c8, frag, typ) in enumerate(jobs):
        o = pos_out + 64 + (5 * i) % 16                       # canaries between the regions, odd alignments
        d[i]["in_off"], d[i]["in_len"], d[i]["slot"] = pos_in, len(pt), slot
        d[i]["out_off"], d[i]["max_frag"], d[i]["type"] = o, frag, typ
        d[i]["out_ctr"] = np.frombuffer(c8, dtype=np.uint8)
        outs.append((pos_out, o, sizes[i]))
        pos_in += _al(len(pt) + 1)
        pos_out = _al(o + sizes[i] + 1)
    ina = np.zeros(max(pos_in, 16) + 128, dtype=np.uint8)
    for i, j in enumerate(jobs):
        ina[int(d[i]["in_off"]):int(d[i]["in_off"]) + len(j[1])] = np.frombuffer(j[1], dtype=np.uint8)
    tin = torch.from_numpy(ina).to(DEV)
    tout = torch.full((pos_out + 128,), CANARY, dtype=torch.uint8, device=DEV)
    recs = torch.zeros(nmax * 40, dtype=torch.uint8, device=DEV)
    res = torch.zeros(nmax * 16, dtype=torch.uint8, device=DEV)
    sres = torch.zeros(len(jobs) * 32, dtype=torch.uint8, device=DEV)
    tivs = _dev(np.frombuffer(ivs, dtype=np.uint8))
    mod = D if dtls else S
    if cbc:
        opts = S.frame_opts(cbc_ivs=tivs if ivs_arg == "own" else ivs_arg)
        n = mod.encrypt_ex(kt, d, len(jobs), tin, tout, recs, res, nmax, sres, opts)
    else:
        n = mod.encrypt(kt, d, len(jobs), tin, tout, recs, res, nmax, sres)
    torch.cuda.synchronize()
    return {"n": n, "out": tout.cpu().numpy(), "sres": sres.cpu().numpy().view(S.STREAM_OUT_RES),
            "recs": recs.cpu().numpy().view(M.BATCH_REC), "res": res.cpu().numpy().view(M.BATCH_RES),
            "outs": outs, "end": pos_out, "ivs": ivs, "firsts": firsts, "counts": counts, "jobs": jobs}


def wire_of(g, i):
    _, o, _ = g["outs"][i]
    return g["out"][o:o + int(g["sres"][i]["out_len"])].tobytes()


def check_send(slots, g, dtls, only=None):
    """a send() result against the model: wire bytes, results, descriptors, IVs, canaries"""
    out, sres, recs, res = g["out"], g["sres"], g["recs"], g["res"]
    assert g["n"] == sum(g["counts"])
    for i, (slot, pt, c8, frag, typ) in enumerate(g["jobs"]):
        if only is not None and i not in only:
            continue
        first = g["firsts"][i]
        p = protector(slots[slot], lambda k: g["ivs"][16 * (first + k):16 * (first + k) + 16])
        r = sres[i]
        start, o, size = g["outs"][i]
        if p is None or (dtls and p.tls13):
            assert (int(r["status"]), int(r["nrec"]), int(r["out_len"])) == (M.ERR_SSL_BAD_INPUT_DATA, 0, 0), i
            wire, wrecs = b"", []
        else:
            st, wire, nrec, c2, wrecs = F._send(p, pt, typ, c8, frag or 16384, dtls)
            assert (int(r["status"]), int(r["nrec"]), int(r["out_len"]), bytes(r["out_ctr"])) == \
                (st, nrec, len(wire), c2), (i, st)
            assert (int(r["first"]), int(r["nparsed"])) == (first, g["counts"][i]), i
            assert out[o:o + len(wire)].tobytes() == wire, i
            hdr = (13 + len(p.cid)) if dtls else 5
            lim = (p.lim.dtls_out_buffer_len - hdr) if dtls else p.lim.out_buf_space
            for k, (ro, dl) in enumerate(wrecs):
                dsc, rr = recs[first + k], res[first + k]
                n = min(frag or 16384, len(pt) - k * (frag or 16384))
                assert (int(dsc["buf_off"]), int(dsc["buf_len"]), int(dsc["data_offset"]), int(dsc["data_len"]),
                        int(dsc["slot"])) == (o + ro, lim, p.head, n, slot), (i, k)
                assert (int(rr["status"]), int(rr["data_offset"]), int(rr["data_len"])) == (0, 0, dl), (i, k)
                if isinstance(slots[slot], R.Key):            # the explicit IV is cbc_ivs[16 j]
                    j = first + k
                    assert wire[ro:ro + 16] == g["ivs"][16 * j:16 * j + 16], (i, k)
        nxt = g["outs"][i + 1][0] if i + 1 < len(g["jobs"]) else g["end"]
        assert (out[start:o] == CANARY).all() and (out[o + len(wire):nxt] == CANARY).all(), \
            f"job {i}: bytes outside its records were written"


def _send_jobs(dtls):
    nslots = 6
    jobs = []
    for i in range(60):
        cnt, frag = [1, 4, 16, 17][i % 4], [1, 15, 16, 17, 1400][i % 5]
        n = cnt * frag - (i % frag if i % 3 == 0 else 0)
        c8 = ctr(1 + i % 3, 1000 * i) if dtls else (i * 7919 + (1 << 33)).to_bytes(8, "big")
        jobs.append((i % nslots, prng_bytes(5000 + i, n), c8, frag, 23 if i % 7 else 22))
    for s in (0, 1, 2):                                       # a full 16 384-byte fragment, and one more byte
        jobs.append((s, prng_bytes(5100 + s, 16384 + (s == 1)), ctr(1, 5) if dtls else bytes(8), 0, 23))
    for s, n in ((0, 15), (1, 17), (2, 1), (0, 16)):          # a whole input of one short record, max_frag 0
        jobs.append((s, prng_bytes(5150 + n, n), ctr(2, 9) if dtls else (77).to_bytes(8, "big"), 0, 23))
    wrap = ctr(4, (1 << 48) - 2) if dtls else ((1 << 64) - 2).to_bytes(8, "big")
    jobs += [(0, prng_bytes(5200, 3000), wrap, 1000, 23), (3 if not dtls else 4, prng_bytes(5201, 3000), wrap, 1000, 23),
             (1, b"", bytes(8), 0, 23)]
    assert len(jobs) == 70
    return jobs


@functools.lru_cache(maxsize=None)
def sent(dtls):
    """the engine's own send output, once per module (the receive tests round-trip it)"""
    slots = DTLS_SLOTS[:6] if dtls else STREAM_SLOTS
    kt = CL.load_table(slots)
    g = send(kt, slots, _send_jobs(dtls), dtls)
    kt.close()
    return g


@pytest.mark.parametrize("dtls", [False, True], ids=["stream", "dtls"])
def test_send_matches_the_model(dtls):
    """70 connections of 1 / 4 / 16 / 17 records of 1, 15, 16, 17, 1 400 and 16 384 bytes over the key matrix
    and two AEAD slots (DTLS: with and without a CID), a counter wrap on a CBC and on an AEAD connection, an
    unloaded slot and an empty input: wire bytes, results, descriptors, each record's IV, canaries."""
    slots = DTLS_SLOTS[:6] if dtls else STREAM_SLOTS
    g = sent(dtls)
    check_send(slots, g, dtls)
    wrapped = [i for i, j in enumerate(g["jobs"]) if int(g["sres"][i]["status"]) == M.ERR_SSL_COUNTER_WRAPPING]
    assert len(wrapped) == 2 and all(int(g["sres"][i]["nrec"]) == 2 for i in wrapped)


@pytest.mark.parametrize("dtls", [False, True], ids=["stream", "dtls"])
def test_send_aead_connections_get_the_plain_calls_bytes(dtls):
    slots = DTLS_SLOTS[:6] if dtls else STREAM_SLOTS
    g = sent(dtls)
    kt = CL.load_table(slots)
    plain = send(kt, slots, _send_jobs(dtls), dtls, cbc=False)
    kt.close()
    seen = 0
    for i, j in enumerate(g["jobs"]):
        a, b = g["sres"][i], plain["sres"][i]
        if isinstance(slots[j[0]], R.Key):                    # the plain call: a CBC slot as never loaded
            if len(j[1]):
                assert (int(b["status"]), int(b["nrec"])) == (M.ERR_SSL_BAD_INPUT_DATA, 0), i
            continue
        seen += 1
        assert (int(a["status"]), int(a["nrec"]), int(a["out_len"]), bytes(a["out_ctr"])) == \
            (int(b["status"]), int(b["nrec"]), int(b["out_len"]), bytes(b["out_ctr"])), i
        assert wire_of(g, i) == wire_of(plain, i), i
    assert seen >= 20


def test_send_without_ivs_is_rejected():
    kt = CL.load_table(STREAM_SLOTS)
    for dtls in (False, True):
        with pytest.raises(S.StreamError) as e:
            send(kt, STREAM_SLOTS, [(0, b"x" * 40, bytes(8), 0, 23)], dtls, ivs_arg=None)
        assert e.value.code == M.ERR_SSL_BAD_INPUT_DATA
    kt.close()


# ---- stream receive ---------------------------------------------------------------
def recv_stream(kt, conns, cbc=True):
    """conns: (slot, bytes, in_ctr int, nb_zero)"""
    d, a, offs, nmax = B.Conns.layout_in(None, conns)
    ta = torch.from_numpy(a).to(DEV)
    recs = torch.zeros(nmax * 40, dtype=torch.uint8, device=DEV)
    res = torch.zeros(nmax * 16, dtype=torch.uint8, device=DEV)
    sres = torch.zeros(len(conns) * 32, dtype=torch.uint8, device=DEV)
    if cbc:
        S.decrypt_ex(kt, d, len(conns), ta, recs, res, nmax, sres, S.frame_opts())
    else:
        S.decrypt(kt, d, len(conns), ta, recs, res, nmax, sres)
    torch.cuda.synchronize()
    return (ta.cpu().numpy(), recs.cpu().numpy().view(M.BATCH_REC), res.cpu().numpy().view(M.BATCH_RES),
            sres.cpu().numpy().view(S.STREAM_IN_RES), offs)


def raw_record(key, content, c8, pad=None, rtype=23):
    """a TLS record sealed by hand under `key` with the padding bytes `pad` (None: the right ones)"""
    ml = R.MACLEN[key.mac]
    body = content if key.etm else content + R._mac(key, c8, rtype, b"\x03\x03", content, b"")
    if pad is None:
        padlen = 15 - len(body) % 16
        pad = bytes([padlen]) * (padlen + 1)
    assert (len(body) + len(pad)) % 16 == 0
    iv = prng_bytes(len(content) + 1, 16)
    ct = iv + R.aes_cbc(key.key, iv, body + pad, True)
    if key.etm:
        ct += R._mac(key, c8, rtype, b"\x03\x03", ct, b"")
    assert len(ct) >= ml
    return bytes([rtype, 3, 3]) + len(ct).to_bytes(2, "big") + ct


@functools.lru_cache(maxsize=None)
def stream_case():
    """the receive connections and what the model makes of them, once per module"""
    g = sent(False)
    conns = []
    for i, (slot, pt, c8, frag, typ) in enumerate(g["jobs"]):
        if STREAM_SLOTS[slot] is not None and len(pt):        # the engine's own output, some with a partial tail
            w = wire_of(g, i)
            conns.append((slot, w + (w[:9] if i % 3 == 0 else b""), int.from_bytes(c8, "big"), i % 2))
    for slot in (0, 1, 2):
        key, p = STREAM_SLOTS[slot], protector(STREAM_SLOTS[slot])
        _, w, _, _ = F.stream_encrypt(p, prng_bytes(600 + slot, 300), 23, bytes(8), 100)
        one = len(w) // 3
        empty = [raw_record(key, b"", k.to_bytes(8, "big")) for k in range(4)]      # (no write call makes these)
        big = F.stream_encrypt(p, prng_bytes(700 + slot, 16384 + 40), 23, bytes(8), 16384)[1]
        over = _abi.MAX_IN_RECORD_CBC - 5 + 1
        conns += [
            (slot, w[:one + 30] + bytes([w[one + 30] ^ 0x80]) + w[one + 31:], 0, 0),                 # tampered
            (slot, w[:len(w) - 1] + bytes([w[-1] ^ 1]), 0, 0),                                        # its last byte
            (slot, w[:one] + _bad_pad(key), 0, 0),                                                    # bad padding
            (slot, w[:one] + bytes([23, 3, 3, 0, 16]) + bytes(16) + w[one:], 0, 0),                   # below 2 blocks
            (slot, w[:one] + bytes([23, 3, 3, 0, R.minlen(key.mac, key.etm) - 1]) +
             prng_bytes(9, R.minlen(key.mac, key.etm) - 1) + w[one:], 0, 0),                          # below minlen
            (slot, b"".join(empty), 0, 0), (slot, b"".join(empty[:2]), 0, 2),                         # zero-length
            (slot, big, 0, 0),                                                                        # largest size
            (slot, w[:one] + bytes([23, 3, 3]) + over.to_bytes(2, "big") + bytes(40), 0, 0),          # one byte over
            (slot, bytes([23, 3, 3]) + (over - 1).to_bytes(2, "big") + prng_bytes(8, over - 1), 0, 0),  # at the limit
            (slot, w + w[:one - 1], 0, 0), (slot, w[:3], 0, 0),                                       # partial
            (slot, bytes([23, 3, 3]) + (_abi.MAX_IN_RECORD - 4).to_bytes(2, "big") + bytes(40), 0, 0),  # (waits: over
        ]                                                                                             # the AEAD limit only)
    for slot in (3, 4):                                       # an AEAD slot keeps the AEAD-only build's limit
        conns.append((slot, bytes([23, 3, 3]) + (_abi.MAX_IN_RECORD - 4).to_bytes(2, "big") + bytes(40), 0, 0))
    want = []
    for slot, data, c0, nbz in conns:
        want.append(F.stream_decrypt(protector(STREAM_SLOTS[slot]), data, c0.to_bytes(8, "big"), nbz))
    return conns, want


def _bad_pad(key):
    """a record whose padding bytes do not all equal the padding length"""
    body = 3 + (0 if key.etm else R.MACLEN[key.mac])
    padlen = 15 - body % 16 + 16                              # two blocks' worth, so there are bytes to spoil
    pad = bytes([padlen]) * (padlen + 1)
    pad = pad[:2] + bytes([pad[2] ^ 0x20]) + pad[3:]
    return raw_record(key, b"abc", (1).to_bytes(8, "big"), pad=pad)


def check_stream(conns, want, got, only=None):
    a, recs, res, sres, offs = got
    for i, ((slot, data, c0, nbz), (w, wrecs, wbuf)) in enumerate(zip(conns, want)):
        if only is not None and slot not in only:
            continue
        g = sres[i]
        assert (int(g["status"]), int(g["nrec"]), int(g["consumed"]), bytes(g["in_ctr"]), int(g["nb_zero"])) == \
            (w["status"], w["nrec"], w["consumed"], w["in_ctr"], w["nb_zero"]), (i, slot, w)
        f = int(g["first"])
        for k, (off, doff, dlen, typ) in enumerate(wrecs):
            rr = res[f + k]
            assert (int(rr["data_offset"]), int(rr["data_len"]), int(rr["type"])) == (doff, dlen, typ), (i, k)
            assert int(recs[f + k]["buf_off"]) == offs[i] + off
            s0 = offs[i] + off + doff
            assert a[s0:s0 + dlen].tobytes() == wbuf[off + doff:off + doff + dlen], (i, k)


# every receive framing path of tests/test_stream_gpu.py (TLSREC_RX_GROUPWALK, TLSREC_GROUPED,
# TLSREC_RX_FUSED_STREAM, TLSREC_RX_RG), and the totals without the mailbox
STREAM_LEGS = [("1", "1", "1", "16", "1"), ("1", "1", "0", "16", "1"), ("1", "1", "0", "8", "1"),
               ("1", "1", "0", "4", "1"), ("0", "0", "0", "16", "1"), ("1", "1", "0", "16", "0")]
STREAM_LEG_IDS = ["one-pass", "groupwalk-16", "groupwalk-8", "groupwalk-4", "r05-framing", "no-mailbox"]


@pytest.mark.parametrize("leg", STREAM_LEGS, ids=STREAM_LEG_IDS)
def test_stream_receive_matches_the_model(leg, monkeypatch):
    """the engine's own send output round-trips (1 .. 17 records a connection), and model-sealed streams end as
    the reference ends them: a tampered MAC, bad padding, a body below minlen, four zero-length records, a
    largest-size record, a record one byte over the CBC limit (BAD_INPUT_DATA), a trailing partial record."""
    for name, v in zip(("TLSREC_RX_GROUPWALK", "TLSREC_GROUPED", "TLSREC_RX_FUSED_STREAM", "TLSREC_RX_RG",
                        "TLSREC_RX_MAILBOX"), leg):
        monkeypatch.setenv(name, v)
    conns, want = stream_case()
    st = [w[0]["status"] for w in want]
    assert {0, M.ERR_SSL_INVALID_MAC, M.ERR_SSL_BAD_INPUT_DATA, M.ERR_SSL_COUNTER_WRAPPING} <= set(st)
    kt = CL.load_table(STREAM_SLOTS)
    check_stream(conns, want, recv_stream(kt, conns))
    kt.close()


def test_stream_receive_aead_connections_get_the_plain_calls_results():
    conns, want = stream_case()
    kt = CL.load_table(STREAM_SLOTS)
    plain = recv_stream(kt, conns, cbc=False)
    kt.close()
    check_stream(conns, want, plain, only=(3, 4))
    for i, (slot, data, c0, nbz) in enumerate(conns):         # ... and a CBC slot as never loaded
        if slot in (0, 1, 2) and want[i][0]["nrec"]:
            assert (int(plain[3][i]["status"]), int(plain[3][i]["nrec"])) == (M.ERR_SSL_BAD_INPUT_DATA, 0), i


def test_stream_read_over_cbc_records():
    """tlsrec_stream_read over the accepted records of CBC connections, against the oracle's read loop"""
    conns, want = stream_case()
    pick = [i for i, c in enumerate(conns) if c[0] in (0, 1, 2) and want[i][0]["nrec"] >= 2][:12]
    conns = [conns[i] for i in pick]
    kt = CL.load_table(STREAM_SLOTS)
    a, recs, res, sres, offs = recv_stream(kt, conns)
    kt.close()
    caps = [[17, 1000, len(c[1]) + 5][k % 3] for k, c in enumerate(conns)]
    req = np.zeros(len(conns), dtype=S.STREAM_READ_REQ)
    pos, outs = 0, []
    for k, cap in enumerate(caps):
        req[k] = (pos, cap, 0)
        outs.append(pos)
        pos += _al(cap) + 128
    ta, tout = torch.from_numpy(a.copy()).to(DEV), torch.zeros(pos, dtype=torch.uint8, device=DEV)
    rres = torch.zeros(len(conns) * 16, dtype=torch.uint8, device=DEV)
    S.read(_dev(sres), len(conns), _dev(recs), _dev(res), ta, req, tout, rres)
    torch.cuda.synchronize()
    a2, o2, rr = ta.cpu().numpy(), tout.cpu().numpy(), rres.cpu().numpy().view(S.STREAM_READ_RES)
    for k, (slot, data, c0, nbz) in enumerate(conns):
        f, nrec = int(sres[k]["first"]), int(sres[k]["nrec"])
        assert nrec >= 2
        wrecs = [(int(recs[f + j]["buf_off"]) - offs[k], int(res[f + j]["data_offset"]), int(res[f + j]["data_len"]),
                  int(res[f + j]["type"])) for j in range(nrec)]
        out, full, left, after = O.stream_read(a[offs[k]:offs[k] + len(data)].tobytes(), wrecs, caps[k])
        assert (int(rr["copied"][k]), int(rr["records"][k]), int(rr["left"][k])) == (len(out), full, left), k
        assert o2[outs[k]:outs[k] + len(out)].tobytes() == out
        assert a2[offs[k]:offs[k] + len(data)].tobytes() == after


# ---- DTLS receive -----------------------------------------------------------------
def recv_dtls(kt, conns, cbc=True):
    """conns: (slot, dict of DtlsState fields, [datagram bytes])"""
    d, dg, ndg, a, offs, nmax = B.Table.layout_in(None, conns)
    ta = torch.from_numpy(a).to(DEV)
    recs = torch.zeros(nmax * 40, dtype=torch.uint8, device=DEV)
    res = torch.zeros(nmax * 16, dtype=torch.uint8, device=DEV)
    disp = torch.zeros(nmax, dtype=torch.int32, device=DEV)
    cres = torch.zeros(len(conns) * 48, dtype=torch.uint8, device=DEV)
    if cbc:
        D.decrypt_ex(kt, d, len(conns), dg, ndg, ta, recs, res, disp, nmax, cres, S.frame_opts())
    else:
        D.decrypt(kt, d, len(conns), dg, ndg, ta, recs, res, disp, nmax, cres)
    torch.cuda.synchronize()
    return (ta.cpu().numpy(), recs.cpu().numpy().view(M.BATCH_REC), res.cpu().numpy().view(M.BATCH_RES),
            disp.cpu().numpy(), cres.cpu().numpy().view(D.DTLS_IN_RES), offs)


def dtls_expect(conns):
    want = []
    for slot, stt, dgs in conns:
        st = F.DtlsState(anti_replay=stt.get("anti_replay", 1))
        for f, v in stt.items():
            setattr(st, f, v)
        want.append((F.dtls_decrypt(protector(DTLS_SLOTS[slot]), st, dgs), st))
    return want


def check_dtls(conns, want, got, only=None):
    """tests/batchlib.check_vs_oracle, against the model"""
    a, recs, res, disp, cres, offs = got
    for i, ((slot, stt, dgs), ((w, wrecs, after), st)) in enumerate(zip(conns, want)):
        if only is not None and slot not in only:
            continue
        g = cres[i]
        assert (int(g["status"]), int(g["nrec"]), int(g["naccepted"]), int(g["dgrams_done"]),
                int(g["invalid_dgrams"])) == (w["status"], w["nrec"], w["naccepted"], w["dgrams_done"],
                                              w["invalid_dgrams"]), (i, slot, w)
        assert (int(g["window_top"]), int(g["window"]), int(g["badmac_seen"]), int(g["nb_zero"])) == \
            (st.window_top, st.window, st.badmac_seen, st.nb_zero), i
        f = int(g["first"])
        for k, (dgi, off, doff, dlen, dsp, typ) in enumerate(wrecs):
            assert int(disp[f + k]) == dsp, (i, k, dsp, int(disp[f + k]))
            assert int(recs[f + k]["buf_off"]) == offs[i][dgi] + off, (i, k)
            if dsp == 0:
                r = res[f + k]
                assert (int(r["data_offset"]), int(r["data_len"]), int(r["type"])) == (doff, dlen, typ), (i, k)
                s0 = offs[i][dgi] + off + doff
                assert a[s0:s0 + dlen].tobytes() == after[dgi][off + doff:off + doff + dlen], (i, k)


def _dgram(slot, seq, epoch=1, n=200, typ=23):
    st, w, _, _ = F.dtls_encrypt(protector(DTLS_SLOTS[slot]), prng_bytes(seq + 31 * slot, n), typ, ctr(epoch, seq), 16384)
    assert st == 0
    return w


def _flip(w, at):
    return w[:at] + bytes([w[at] ^ 0x10]) + w[at + 1:]


@functools.lru_cache(maxsize=None)
def dtls_case():
    g = sent(True)
    conns = []
    for i, (slot, pt, c8, frag, typ) in enumerate(g["jobs"]):      # the engine's own datagrams
        p = protector(DTLS_SLOTS[slot])
        if p is None or not len(pt) or int(g["sres"][i]["nrec"]) == 0:
            continue
        hdr, first = 13 + len(p.cid), g["firsts"][i]
        grams = []
        for k in range(int(g["sres"][i]["nrec"])):
            s = int(g["recs"][first + k]["buf_off"]) - hdr
            grams.append(g["out"][s:s + hdr + int(g["res"][first + k]["data_len"])].tobytes())
        if len(grams) >= 3:                                        # two records packed into one datagram
            grams = [grams[0] + grams[1]] + grams[2:]
        conns.append((slot, {"in_epoch": int.from_bytes(c8[:2], "big"), "cid_len": len(p.cid)}, grams))
    for slot in (0, 1, 2, 4):
        cl = len(DTLS_SLOTS[slot].cid) if isinstance(DTLS_SLOTS[slot], R.Key) else 0
        base = {"in_epoch": 1, "cid_len": cl}
        r = [_dgram(slot, k) for k in range(12)]
        at = 13 + cl + 40
        conns += [
            # replays, an old and an early epoch, a bad MAC that drops the rest of a two-record datagram
            (slot, dict(base), [r[0], r[0], _dgram(slot, 50, epoch=0), _dgram(slot, 60, epoch=2),
                                _flip(r[2], at) + r[3], r[3], r[4] + r[5], r[5], r[2]]),
            (slot, dict(base), [_flip(r[6], at), r[6], r[6]]),
            (slot, dict(base, badmac_limit=2), [r[0], _flip(r[1], at), r[2], _flip(r[3], at), r[4], r[5]]),
            (slot, dict(base, badmac_limit=3, badmac_seen=1), [_flip(r[1], at), r[2]]),
            (slot, dict(base, window_top=9, window=0b1011), [r[9], r[8], r[7], r[6], r[10]]),
            (slot, dict(base, anti_replay=0), [r[3], r[3], r[1]]),
            (slot, dict(base), [r[0] + b"\x17\xfe\xfd", r[1]]), (slot, dict(base), [r[0], b"", r[1]]),
            (slot, dict(base), [r[0] + bytes(_abi.DTLS_MAX_DATAGRAM_CBC)]),          # read truncated, by slot kind
        ]
    big = _dgram(2, 7, n=16384)                               # a largest-size record: past the AEAD build's datagram
    assert len(big) > _abi.DTLS_MAX_DATAGRAM
    conns.append((2, {"in_epoch": 1, "cid_len": 5}, [big, _dgram(2, 8)]))
    # unexpected CID: a record without one, and one with another CID, ignored and fatal
    for ign in (1, 0):
        conns.append((1, {"in_epoch": 1, "cid_len": 3, "ignore_unexpected_cid": ign},
                      [_dgram(1, 1), _dgram(3, 2), _dgram(6, 3), _dgram(1, 4)]))
    return conns, dtls_expect(conns)


# every path of tests/test_dtls_gpu.py and tests/test_dtls_stash_gpu.py (TLSREC_DTLS_STASH, TLSREC_GROUPED,
# TLSREC_RX_FUSED), and the totals without the mailbox
DTLS_LEGS = [(None, "1", "1", "1"), (None, "0", "1", "1"), ("0", "1", "1", "1"), ("0", "0", "1", "1"),
             (None, "1", "0", "1"), (None, "0", "0", "1"), (None, "1", "1", "0")]
DTLS_LEG_IDS = ["stash-grouped", "stash-bucket", "nostash-grouped", "nostash-bucket", "three-kernels",
                "bucket-pass-3-kernels", "no-mailbox"]


def _dtls_leg(monkeypatch, leg):
    stash, grouped, fused, mbox = leg
    if stash is None:
        monkeypatch.delenv("TLSREC_DTLS_STASH", raising=False)
    else:
        monkeypatch.setenv("TLSREC_DTLS_STASH", stash)
    monkeypatch.setenv("TLSREC_GROUPED", grouped)
    monkeypatch.setenv("TLSREC_RX_FUSED", fused)
    monkeypatch.setenv("TLSREC_RX_MAILBOX", mbox)


@pytest.mark.parametrize("leg", DTLS_LEGS, ids=DTLS_LEG_IDS)
def test_dtls_receive_matches_the_model(leg, monkeypatch):
    """the engine's own datagrams round-trip (with two-record datagrams), and model-sealed ones end as the
    reference ends them: replays, an old epoch, a bad MAC that drops the rest of its datagram, badmac_limit,
    unexpected CIDs, a datagram longer than the AEAD-only build's buffer (stash depth 16: the mean connection
    holds more than 4 datagrams)."""
    _dtls_leg(monkeypatch, leg)
    conns, want = dtls_case()
    assert sum(len(c[2]) for c in conns) > 4 * len(conns)
    kt = CL.load_table(DTLS_SLOTS)
    check_dtls(conns, want, recv_dtls(kt, conns))
    kt.close()


def test_dtls_receive_aead_connections_get_the_plain_calls_results():
    conns, want = dtls_case()
    kt = CL.load_table(DTLS_SLOTS)
    plain = recv_dtls(kt, conns, cbc=False)
    kt.close()
    check_dtls(conns, want, plain, only=(4, 5))
    for i, (slot, stt, dgs) in enumerate(conns):              # ... and a CBC slot as never loaded
        if isinstance(DTLS_SLOTS[slot], R.Key):
            assert (int(plain[4][i]["status"]), int(plain[4][i]["nrec"])) == (M.ERR_SSL_BAD_INPUT_DATA, 0), i


@pytest.mark.parametrize("leg", DTLS_LEGS[:1] + DTLS_LEGS[4:5], ids=DTLS_LEG_IDS[:1] + DTLS_LEG_IDS[4:5])
def test_dtls_300_connections(leg, monkeypatch):
    """300 connections (two tiles of the one-pass kernel's look-back) of 0 .. 3 datagrams of one or two
    records (stash depth 4), replays, other epochs, bad MACs and a trailing byte among them"""
    _dtls_leg(monkeypatch, leg)
    rng = np.random.default_rng(41)
    conns = []
    for i in range(300):
        slot = i % 6
        if slot == 3:
            slot = 0
        cl = len(DTLS_SLOTS[slot].cid) if isinstance(DTLS_SLOTS[slot], R.Key) else 0
        seq, grams = int(rng.integers(1, 1000)), []
        for _ in range(int(rng.integers(0, 4))):
            g = _dgram(slot, seq, n=int(rng.integers(1, 90)))
            seq += 1
            u = rng.random()
            if u < 0.2:
                g += _dgram(slot, seq, n=int(rng.integers(1, 40)))
                seq += 1
            elif u < 0.3:
                g = _flip(g, 13 + cl + 20)
            elif u < 0.35:
                g += b"\x17"
            elif u < 0.4:
                g = _dgram(slot, seq - 1, epoch=2, n=30)
            grams.append(g)
        if grams and rng.random() < 0.1:
            grams.append(grams[0])
        conns.append((slot, {"in_epoch": 1, "cid_len": cl}, grams))
    kt = CL.load_table(DTLS_SLOTS)
    check_dtls(conns, dtls_expect(conns), recv_dtls(kt, conns))
    kt.close()


# ---- launch log --------------------------------------------------------------------
def test_framed_calls_reach_the_cbc_kernel_in_identity_order(launch_log, monkeypatch):  # noqa: F811
    """a framed call with TLSREC_FRAME_CBC launches the CBC kernels over the grouped records without the bucket
    pass, send through the copy path; the plain call launches none"""
    for name in ("TLSREC_GROUPED", "TLSREC_STREAM_SRC"):
        monkeypatch.delenv(name, raising=False)
    kt = CL.load_table(STREAM_SLOTS)
    jobs = [(s, prng_bytes(40 + s, 700), bytes(8), 100, 23) for s in range(5)]
    macs = (1 << R.MAC_SHA1) | (1 << R.MAC_SHA256) | (1 << R.MAC_SHA384)
    for dtls in (False, True):
        launch_log.reset()
        g = send(kt, STREAM_SLOTS, jobs, dtls)
        assert launch_log(_abi.LOG_SEND_FRAME) == [(_abi.LOG_SEND_FRAME, 0, int(dtls), 0, 0)]
        assert launch_log(_abi.LOG_BUCKET) == [(_abi.LOG_BUCKET, 0, 0, 0, 0)]
        assert launch_log(_abi.LOG_CBC) == [(_abi.LOG_CBC, 0, macs, 0b11, 0)]
        check_send(STREAM_SLOTS, g, dtls)
        launch_log.reset()
        send(kt, STREAM_SLOTS, jobs, dtls, cbc=False)
        assert launch_log(_abi.LOG_BUCKET) == [(_abi.LOG_BUCKET, 0, 0, 0, 0)] and launch_log(_abi.LOG_CBC) == []
    g = send(kt, STREAM_SLOTS, jobs, False)
    conns = [(s, wire_of(g, s), 0, 0) for s in range(5)]
    launch_log.reset()
    got = recv_stream(kt, conns)
    assert launch_log(_abi.LOG_BUCKET) == [(_abi.LOG_BUCKET, 0, 0, 0, 0)]
    assert launch_log(_abi.LOG_CBC) == [(_abi.LOG_CBC, 1, macs, 0b11, 0)]
    assert [int(x) for x in got[3]["status"]] == [0] * 5 and [int(x) for x in got[3]["nrec"]] == [7] * 5
    launch_log.reset()
    recv_stream(kt, conns, cbc=False)
    assert launch_log(_abi.LOG_CBC) == []
    kt.close()
