"""ARIA-CBC / Camellia-CBC + HMAC records on the GPU, bit-exact against
tests/cbc_alt_ref.py (the record model of tests/cbc_ref.py around OpenSSL's
ARIA / Camellia) and, for the AEAD records of a mixed batch, against oracle/.
Every record of every batch is compared."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

import mbedtls_amd as M  # noqa: E402
from mbedtls_amd import _abi  # noqa: E402
from mbedtls_amd import cbc as C  # noqa: E402
from mbedtls_amd import tls12 as T  # noqa: E402
from tests import batchlib as B  # noqa: E402
from tests import cbc_alt_lib as L  # noqa: E402
from tests import cbc_alt_ref as A  # noqa: E402
from tests import cbc_frames_ref as F  # noqa: E402
from tests import cbc_ref as R  # noqa: E402
from tests import test_cbc_frames_gpu as FG  # noqa: E402  (its send / receive harness)
from tests import tls12_ref  # noqa: E402
from tests.batchlib import launch_log  # noqa: E402,F401  (fixture)
from tests.prng import prng_bytes  # noqa: E402

DEV = torch.device("cuda")
ARIA128, ARIA256, CAM128, CAM256 = sorted(A.KEYLEN)
# block edges, the SHA-256 / SHA-512 padding edges behind a 13-byte header, the largest record
LENGTHS = [0, 1, 15, 16, 17, 31, 32, 47, 48, 255, 256, 257, 1400, 16384]


def _variant_bit(cipher, mac):
    """the launch log's p3 bit of an ARIA / Camellia variant"""
    return 1 << (3 * (cipher - ARIA128) + (mac - 1))


def _sealed(recs, want):
    return [B.Rec(r.slot, bytearray(w[5]), w[1], w[2], r.ctr, w[3], r.ver) for r, w in zip(recs, want)]


@pytest.mark.parametrize("inplace", [True, False])
def test_round_trip_and_known_answers(inplace):
    """4 suites x 2 MAC orders x 14 lengths: the wire bytes equal the model's, and decrypt back"""
    slots = [L.make_key(100 + i, c, m, e) for i, (c, m, e) in enumerate(L.ALT_KEYS)]
    recs = [L.plain_rec(s, n, 1000 * s + n) for s in range(len(slots)) for n in LENGTHS]
    run = L.Run(slots, recs)
    kt = L.load_table(slots)
    want = run.expected(False)
    assert all(w[0] == 0 for w in want)
    out, res = run.gpu(False, inplace=inplace, kt=kt)
    bad = run.compare(False, out, res, inplace, want)
    assert not bad, bad[:5]
    sealed = _sealed(recs, want)
    back = L.Run(slots, sealed)
    out, res = back.gpu(True, inplace=inplace, kt=kt)
    bad = back.compare(True, out, res, inplace)
    assert not bad, bad[:5]
    for i, r in enumerate(recs):                            # and it is the plaintext we started from
        o = back.offs[i] + int(res[i]["data_offset"])
        assert int(res[i]["data_len"]) == r.data_len
        assert bytes(out[o:o + r.data_len]) == bytes(r.buf[r.data_offset:r.data_offset + r.data_len])
    kt.close()


@pytest.mark.parametrize("cipher,mac", [(ARIA128, R.MAC_SHA256), (CAM256, R.MAC_SHA384)])
def test_padding_and_mac_sweep(cipher, mac):
    """MAC-then-encrypt: every pad value 0..255 on one record length, and a flipped bit in every byte of the
    MAC, the padding and the last ciphertext block; statuses and result fields are the model's"""
    key = L.make_key(7, cipher, mac, 0)
    ml = R.MACLEN[mac]
    ctr, ver = bytes(8), b"\x03\x03"
    content = bytes([42]) * 19
    padlen = 15 - (len(content) + ml) % 16
    pre = content + R._mac(key, ctr, 23, ver, content, b"") + bytes([padlen]) * (padlen + 1)
    iv = bytes([0x55]) * 16
    cases = [(pre, 0)]
    for v in range(256):                                    # the pad-value loop
        b = bytearray(pre)
        b[len(b) - padlen - 1:] = bytes([v]) * (padlen + 1)
        cases.append((bytes(b), 0 if v == padlen else M.ERR_SSL_INVALID_MAC))
    for i in range(len(content), len(pre)):                 # a bit of the MAC and of the padding
        b = bytearray(pre)
        b[i] ^= 1
        cases.append((bytes(b), M.ERR_SSL_INVALID_MAC))
    wires = [iv + A.block_cbc(cipher, key.key, iv, p, True) for p, _ in cases]
    for i in range(16):                                     # a bit of the last ciphertext block
        w = bytearray(wires[0])
        w[len(w) - 16 + i] ^= 0x10
        wires.append(bytes(w))
        cases.append((None, M.ERR_SSL_INVALID_MAC))
    recs = [B.Rec(0, bytearray(w), 0, len(w), ctr, 23) for w in wires]
    run = L.Run([key], recs)
    want = run.expected(True)
    assert [w[0] for w in want] == [st for _, st in cases]  # the model agrees with the construction
    out, res = run.gpu(True)
    bad = run.compare(True, out, res, True, want)
    assert not bad, (len(bad), bad[:5])


@pytest.mark.parametrize("etm", [0, 1])
def test_length_checks(etm):
    """data_len below 32, below 16 + maclen + 1, not a multiple of 16: all INVALID_MAC"""
    slots = [L.make_key(20, ARIA256, R.MAC_SHA384, etm), L.make_key(21, CAM128, R.MAC_SHA256, etm)]
    recs = []
    for s, k in enumerate(slots):
        ml = R.MACLEN[k.mac]
        good = L.sealed_rec(k, s, 40, 5 + s)
        for n in sorted({0, 1, 16, 31, 32, 16 + ml, 16 + ml + 1, good.data_len - 1, good.data_len - 16 + 1,
                         good.data_len - 15, good.data_len}):
            if n <= good.data_len:
                recs.append(B.Rec(s, bytearray(good.buf), good.data_offset, n, good.ctr, 23))
    run = L.Run(slots, recs)
    want = run.expected(True)
    assert sum(w[0] == M.ERR_SSL_INVALID_MAC for w in want) >= len(want) - len(slots)
    assert [w[0] for w in want].count(0) == len(slots)
    out, res = run.gpu(True)
    bad = run.compare(True, out, res, True, want)
    assert not bad, bad[:5]


def test_little_space_on_encrypt():
    """BUFFER_TOO_SMALL at ssl_msg.c:909, :1098, :1116 and :1199: every buffer length from none to ample,
    and short heads"""
    slots = [L.make_key(40 + i, c, A.MAC_OF[c], e) for i, (c, e) in
             enumerate(((ARIA128, 0), (ARIA128, 1), (CAM256, 0), (CAM256, 1)))]
    recs = []
    for s in range(len(slots)):
        for n in (0, 5, 16, 31):
            for room in range(0, 16 + 48 + 2):
                recs.append(L.plain_rec(s, n, 7 * s + n, head=16, tail=room))
            for head in (0, 8, 15, 16):
                recs.append(L.plain_rec(s, n, 9 * s + n, head=head, tail=80))
    run = L.Run(slots, recs)
    want = run.expected(False)
    st = [w[0] for w in want]
    assert st.count(M.ERR_SSL_BUFFER_TOO_SMALL) > 100 and st.count(0) > 100
    assert any(a == M.ERR_SSL_BUFFER_TOO_SMALL and b == 0 for a, b in zip(st, st[1:]))
    out, res = run.gpu(False)
    bad = run.compare(False, out, res, True, want)
    assert not bad, bad[:5]


def test_encrypt_then_mac_tampering():
    """a flipped IV, ciphertext or MAC byte: INVALID_MAC with the reference's fields, nothing outside the
    record buffer written"""
    slots = [L.make_key(60, ARIA256, R.MAC_SHA384, 1), L.make_key(61, CAM128, R.MAC_SHA256, 1)]
    recs = []
    for s, k in enumerate(slots):
        good = L.sealed_rec(k, s, 64, 70 + s)
        recs.append(good)
        for pos in (good.data_offset, good.data_offset + 16, good.data_offset + 40,
                    good.data_offset + good.data_len - R.MACLEN[k.mac], good.data_offset + good.data_len - 1):
            b = bytearray(good.buf)
            b[pos] ^= 0x80
            recs.append(B.Rec(s, b, good.data_offset, good.data_len, good.ctr, 23))
    run = L.Run(slots, recs)
    want = run.expected(True)
    assert [w[0] for w in want].count(M.ERR_SSL_INVALID_MAC) == 5 * len(slots)
    for inplace in (True, False):
        out, res = run.gpu(True, inplace=inplace)
        bad = run.compare(True, out, res, inplace, want)
        assert not bad, bad[:5]


def test_dtls12_with_and_without_cid():
    """epoch + 48-bit sequence in ctr, version FE FD; CID slots wrap the content in a DTLSInnerPlaintext; a
    wrong CID is UNEXPECTED_CID, an all-zero inner plaintext INVALID_RECORD"""
    ver = b"\xfe\xfd"
    cid = bytes(range(0x10, 0x15))
    keys = [(ARIA128, R.MAC_SHA256, 0), (ARIA256, R.MAC_SHA384, 1), (CAM128, R.MAC_SHA256, 1),
            (CAM256, R.MAC_SHA384, 0)]
    slots = [L.make_key(80 + i, c, m, e, cid=(cid if i % 2 == 0 else b"") if i < 3 else bytes(range(32)))
             for i, (c, m, e) in enumerate(keys)]
    ctr = lambda i: (1).to_bytes(2, "big") + (1000 + i).to_bytes(6, "big")
    plain = [L.plain_rec(s, n, 3 * s + n, tail=128, ver=ver, ctr=ctr(n)) for s in range(len(slots))
             for n in (0, 1, 15, 16, 64)]
    run = L.Run(slots, plain)
    want = run.expected(False)
    assert all(w[0] == 0 for w in want)
    assert {w[3] for w in want} == {23, M.MSG_CID}
    out, res = run.gpu(False)
    bad = run.compare(False, out, res, True, want)
    assert not bad, bad[:5]
    sealed = [B.Rec(r.slot, bytearray(w[5]), w[1], w[2], r.ctr, w[3], ver, slots[r.slot].cid)
              for r, w in zip(plain, want)]
    s0 = sealed[0]
    sealed.append(B.Rec(0, bytearray(s0.buf), s0.data_offset, s0.data_len, s0.ctr, s0.type, ver, b"\x10\x11\x12\x13\x99"))
    sealed.append(B.Rec(0, bytearray(s0.buf), s0.data_offset, s0.data_len, s0.ctr, s0.type, ver, b""))
    s1 = next(r for r in sealed if r.slot == 1)
    sealed.append(B.Rec(1, bytearray(s1.buf), s1.data_offset, s1.data_len, s1.ctr, s1.type, ver, cid))
    k0 = slots[0]                                           # an inner plaintext of zeros only, sealed by hand
    zero = bytearray(L.plain_rec(0, 0, 5, tail=128, ver=ver, ctr=ctr(7)).buf)
    inner = bytes(16)
    body = inner + R._mac(k0, ctr(7), M.MSG_CID, ver, inner, cid)
    padlen = 15 - len(body) % 16
    body += bytes([padlen]) * (padlen + 1)
    zero[16:16 + len(body)] = A.block_cbc(k0.cipher, k0.key, bytes(zero[:16]), body, True)
    sealed.append(B.Rec(0, zero, 0, 16 + len(body), ctr(7), M.MSG_CID, ver, cid))
    back = L.Run(slots, sealed)
    want = back.expected(True)
    assert [w[0] for w in want[-4:]] == [M.ERR_SSL_UNEXPECTED_CID] * 3 + [M.ERR_SSL_INVALID_RECORD]
    assert all(w[0] == 0 for w in want[:-4])
    out, res = back.gpu(True)
    bad = back.compare(True, out, res, True, want)
    assert not bad, bad[:5]


def test_key_passes_over_one_shuffled_batch(launch_log):  # noqa: F811
    """1 100 records (three workgroups, the last partial) over 12 slots in random order: the four suites, two
    AES-CBC suites, AES-128-GCM, ChaCha20-Poly1305, ARIA-128-CCM, an unloaded slot, and two suites a second
    time with 0 and 1 records; one record in eight tampered.  Each present variant launched once."""
    aead = B.random_slots(5, [M.CIPHER_AES_128_GCM, M.CIPHER_CHACHA20_POLY1305, M.CIPHER_ARIA_128_CCM],
                          [M.VERSION_TLS1_2], 3)
    slots = [L.make_key(200 + i, c, m, e) for i, (c, m, e) in enumerate(L.ALT_KEYS[::2])]       # 0..3, etm 0
    slots += [L.make_key(210, R.CIPHER_AES_128_CBC, R.MAC_SHA256, 1), L.make_key(211, R.CIPHER_AES_256_CBC, R.MAC_SHA1, 0)]
    slots += list(aead) + [None, L.make_key(212, CAM128, R.MAC_SHA256, 1), L.make_key(213, ARIA256, R.MAC_SHA384, 1)]
    assert len(slots) == 12
    rng = np.random.default_rng(11)
    pick = rng.integers(0, 10, size=1100)                   # slots 0..9 at random: every wave sees several
    pick[500] = 11                                          # slot 11: one record; slot 10: none
    assert 10 not in pick and list(pick).count(11) == 1
    lens = rng.integers(0, 65, size=1100)
    plain = [L.plain_rec(int(s), int(n), 31 * j, head=24) for j, (s, n) in enumerate(zip(pick, lens))]
    run = L.Run(slots, plain)
    want = run.expected(False)
    assert [w[0] for w in want].count(M.ERR_SSL_BAD_INPUT_DATA) == list(pick).count(9)
    kt = L.load_table(slots)
    launch_log.reset()
    out, res = run.gpu(False, kt=kt)
    bad = run.compare(False, out, res, True, want)
    assert not bad, (len(bad), bad[:5])
    present = sum(_variant_bit(c, m) for c, m in A.SUITES)
    cbc = launch_log(_abi.LOG_CBC)
    assert len(cbc) == 1 and cbc[0][1:] == (0, (1 << R.MAC_SHA1) | (1 << R.MAC_SHA256) | (1 << R.MAC_SHA384), 0b11, present)
    assert {_abi.LOG_GCM, _abi.LOG_CHACHA, _abi.LOG_CCM} <= {e[0] for e in launch_log()}
    assert launch_log(_abi.LOG_BUCKET)[-1][1] == 1
    sealed = [B.Rec(r.slot, bytearray(w[5]), w[1], w[2], r.ctr, w[3], r.ver) for r, w in zip(plain, want)]
    for j in range(0, len(sealed), 8):                      # one record in eight: a flipped byte near the end
        r = sealed[j]
        if want[j][0] == 0:
            r.buf[r.data_offset + r.data_len - 3] ^= 0x04
    back = L.Run(slots, sealed)
    wantd = back.expected(True)
    st = [w[0] for w in wantd]
    assert st.count(M.ERR_SSL_INVALID_MAC) > 100 and st.count(0) > 800
    launch_log.reset()
    out, res = back.gpu(True, kt=kt)
    bad = back.compare(True, out, res, True, wantd)
    assert not bad, (len(bad), bad[:5])
    cbc = launch_log(_abi.LOG_CBC)
    assert len(cbc) == 1 and cbc[0][1] == 1 and cbc[0][4] == present
    kt.close()


def test_launch_log_tells_the_variants_apart(launch_log):  # noqa: F811
    for c, m in A.SUITES:
        key = L.make_key(250 + c, c, m, 0)
        run = L.Run([key], [L.plain_rec(0, 20, c)])
        launch_log.reset()
        out, res = run.gpu(False)
        assert not run.compare(False, out, res)
        assert launch_log(_abi.LOG_CBC)[-1][1:] == (0, 1 << m, 0b01, _variant_bit(c, m))
    run = L.Run([L.make_key(260, R.CIPHER_AES_128_CBC, R.MAC_SHA256, 0)], [L.plain_rec(0, 20, 3)])
    launch_log.reset()
    run.gpu(False)
    assert launch_log(_abi.LOG_CBC)[-1][1:] == (0, 1 << R.MAC_SHA256, 0b01, 0)      # AES alone: as it always was


def test_slot_reloads_across_every_kind():
    """ARIA-256-CBC -> AES-128-GCM -> Camellia-128-CBC -> AES-256-CBC -> ARIA-128-CBC in one slot: records
    under each owner match the model, and a record sealed for the previous owner fails"""
    owners = [L.make_key(300, ARIA256, R.MAC_SHA384, 0),
              B.random_slots(9, [M.CIPHER_AES_128_GCM], [M.VERSION_TLS1_2], 1)[0],
              L.make_key(301, CAM128, R.MAC_SHA256, 1), L.make_key(302, R.CIPHER_AES_256_CBC, R.MAC_SHA384, 0),
              L.make_key(303, ARIA128, R.MAC_SHA256, 0)]
    other = L.make_key(304, CAM256, R.MAC_SHA384, 1)
    kt = L.load_table([owners[0], other])
    prev_sealed = None
    for s in owners:
        if isinstance(s, R.Key):
            C.load(kt, C.key_material(s.cipher, s.mac, s.etm, s.key, s.mac_key), first=0)
        else:
            kt.load(M.key_material(*s), first=0)
        recs = [L.plain_rec(i % 2, n, n, head=24) for i, n in enumerate((0, 1, 33, 64, 47, 48))]
        run = L.Run([s, other], recs)
        want = run.expected(False)
        out, res = run.gpu(False, kt=kt)
        bad = run.compare(False, out, res, True, want)
        assert not bad, (type(s), bad[:5])
        sealed = [x for x in _sealed(recs, want) if x.slot == 0]
        back = L.Run([s, other], sealed + (prev_sealed or []))
        out, res = back.gpu(True, kt=kt)
        bad = back.compare(True, out, res)
        assert not bad, (type(s), bad[:5])
        assert all(int(r["status"]) == 0 for r in res[:len(sealed)])
        assert all(int(r["status"]) != 0 for r in res[len(sealed):])       # the previous owner's records
        prev_sealed = sealed
    kt.close()


def test_unreached_record_fails_closed():
    """the skip-record hook on a record of a new slot leaves INTERNAL_ERROR"""
    with _abi.use_library() as lib:
        f = lib.tlsrec__test_skip_record
        f.argtypes, f.restype = [ctypes.c_uint32], None
        try:
            for slots in ([L.make_key(400, CAM128, R.MAC_SHA256, 0)],
                          [L.make_key(401 + i, c, m, e) for i, (c, m, e) in enumerate(L.ALT_KEYS[1::2])]):
                recs = [L.plain_rec(i % len(slots), 50 + i, i) for i in range(12)]
                run = L.Run(slots, recs)
                f(5)
                out, res = run.gpu(False)
                assert int(res[5]["status"]) == M.ERR_SSL_INTERNAL_ERROR
                o = run.offs[5]
                assert bytes(out[o:o + len(recs[5].buf)]) == bytes(recs[5].buf)
                bad = [b for b in run.compare(False, out, res) if not b.startswith("rec 5 ")]
                assert not bad, bad[:5]
        finally:
            f(0xFFFFFFFF)


def test_host_batch():
    slots = [L.make_key(500 + i, c, m, e) for i, (c, m, e) in enumerate(L.ALT_KEYS[::3])] + \
            [L.make_key(510, R.CIPHER_AES_128_CBC, R.MAC_SHA1, 0)]
    recs = [L.plain_rec(i % len(slots), n, 40 + i) for i, n in enumerate((0, 16, 64, 1400, 4000, 17, 33, 15))]
    run = L.Run(slots, recs)
    want = run.expected(False)
    kt = L.load_table(slots)
    out, res = run.gpu(False, kt=kt, host=True)
    bad = run.compare(False, out, res, True, want)
    assert not bad, bad[:5]
    back = L.Run(slots, _sealed(recs, want))
    out, res = back.gpu(True, kt=kt, host=True)
    bad = back.compare(True, out, res)
    assert not bad, bad[:5]
    kt.close()


# ---- the stream and DTLS layers' _ex calls -------------------------------------------------
FRAME_SLOTS = [L.make_key(601, ARIA128, R.MAC_SHA256, 0), L.make_key(602, ARIA256, R.MAC_SHA384, 1),
               L.make_key(603, CAM128, R.MAC_SHA256, 1), L.make_key(604, CAM256, R.MAC_SHA384, 0),
               L.make_key(605, R.CIPHER_AES_128_CBC, R.MAC_SHA1, 0),
               (M.CIPHER_AES_128_GCM, M.VERSION_TLS1_2, prng_bytes(606, 16), prng_bytes(607, 12), 0)]


def _frame_jobs(dtls):
    jobs = []
    for s in range(6):                                      # 1..5 records a connection, the last one short
        cnt, frag = 1 + (s + 2) % 5, [64, 33, 16, 48, 17, 64][s]
        c8 = FG.ctr(1, 100 * s) if dtls else (s * 7919 + (1 << 33)).to_bytes(8, "big")
        jobs.append((s, prng_bytes(6000 + s, cnt * frag - s % 3), c8, frag, 23))
    jobs.append((1, prng_bytes(6100, 16384), FG.ctr(1, 5) if dtls else bytes(8), 0, 23))      # at the CBC limits
    return jobs


@pytest.mark.parametrize("dtls", [False, True], ids=["stream", "dtls"])
def test_stream_and_dtls_ex_calls(dtls):
    """6 connections (the four suites, AES-CBC, AES-GCM) and a 16 384-byte record: the send call's wire bytes,
    results, descriptors and IVs are the framing model's over the record model, and the receive call opens the
    engine's own output as the model does"""
    kt = L.load_table(FRAME_SLOTS)
    with A.as_model():
        g = FG.send(kt, FRAME_SLOTS, _frame_jobs(dtls), dtls)
        FG.check_send(FRAME_SLOTS, g, dtls)
        assert all(int(r["status"]) == 0 for r in g["sres"])
        assert {int(r["nrec"]) for r in g["sres"][:6]} == {1, 2, 3, 4, 5}
        wires = [FG.wire_of(g, i) for i in range(len(g["jobs"]))]
        if not dtls:
            conns = [(j[0], w, int.from_bytes(j[2], "big"), 0) for j, w in zip(g["jobs"], wires)]
            want = [F.stream_decrypt(FG.protector(FRAME_SLOTS[s]), w, c.to_bytes(8, "big"), nbz)
                    for s, w, c, nbz in conns]
            assert all(w[0]["status"] == 0 and w[0]["nrec"] == int(r["nrec"]) for w, r in zip(want, g["sres"]))
            FG.check_stream(conns, want, FG.recv_stream(kt, conns))
        else:
            conns, want = [], []
            for i, (j, w) in enumerate(zip(g["jobs"], wires)):
                # one record a datagram, as the send call laid them out
                f, n = int(g["sres"][i]["first"]), int(g["sres"][i]["nrec"])
                _, o, _ = g["outs"][i]
                dgs, pos = [], 0
                for k in range(n):
                    ln = 13 + int.from_bytes(w[pos + 11:pos + 13], "big")
                    dgs.append(w[pos:pos + ln])
                    pos += ln
                assert pos == len(w)
                stt = {"in_epoch": 1}
                conns.append((j[0], stt, dgs))
                st = F.DtlsState(anti_replay=1)
                st.in_epoch = 1
                want.append((F.dtls_decrypt(FG.protector(FRAME_SLOTS[j[0]]), st, dgs), st))
            assert all(w[0][0]["status"] == 0 and w[0][0]["naccepted"] == int(r["nrec"])
                       for w, r in zip(want, g["sres"]))
            FG.check_dtls(conns, want, FG.recv_dtls(kt, conns))
    kt.close()


# ---- calls that refuse CBC slots: a new slot is a never-loaded slot ---------------------------
_AEAD = (M.CIPHER_AES_128_GCM, M.VERSION_TLS1_2, bytes(16), bytes(16), 0)


def _same(a, b, skip=()):
    return all(np.array_equal(a[f], b[f]) for f in a.dtype.names if f not in skip)


@pytest.mark.parametrize("cipher", [ARIA256, CAM128])
def test_plain_stream_and_dtls_calls_treat_a_new_slot_as_unloaded(cipher):
    key = L.make_key(700, cipher, A.MAC_OF[cipher], 0)
    kt = L.load_table([key, None])
    c = B.Conns.__new__(B.Conns)
    c.slots, c.kt, c.ot = [_AEAD, _AEAD], kt, []
    data = prng_bytes(3, 300)
    (s0, o0), (s1, o1) = c.encrypt([(0, data, 5, 100, 23), (1, data, 5, 100, 23)])
    assert _same(s0, s1, skip=("first",)) and o0 == o1 and c.last_regions[0] == c.last_regions[1]
    assert int(s0["status"]) != 0
    r = L.sealed_rec(key, 0, 64, 1, ctr=(7).to_bytes(8, "big"))
    body = bytes(r.buf[r.data_offset:r.data_offset + r.data_len])
    wire = bytes([23, 3, 3]) + len(body).to_bytes(2, "big") + body
    a, recs, res, sres, offs = c.decrypt([(0, wire, 7, 0), (1, wire, 7, 0)])
    assert _same(sres[0], sres[1], skip=("first",)), (sres[0], sres[1])
    assert int(sres[0]["status"]) != 0 and int(sres[0]["nrec"]) == 0
    assert bytes(a[offs[0]:offs[0] + len(wire)]) == bytes(a[offs[1]:offs[1] + len(wire)])
    t = B.Table.__new__(B.Table)
    t.slots, t.gran_of, t.kt, t.ot = [(M.CIPHER_AES_128_GCM, bytes(16), bytes(16), b"")] * 2, {}, kt, []
    ctr = (1).to_bytes(2, "big") + (9).to_bytes(6, "big")
    (d0, p0, _, _), (d1, p1, _, _) = t.encrypt([(0, data, ctr, 100, 23), (1, data, ctr, 100, 23)])
    assert _same(d0, d1, skip=("first",)) and p0 == p1
    assert int(d0["status"]) == M.ERR_SSL_BAD_INPUT_DATA
    kt.close()


def test_ticket_calls_treat_a_new_slot_as_unloaded():
    from mbedtls_amd import ticket as TK
    kt = L.load_table([L.make_key(710, CAM256, R.MAC_SHA384, 0), None])
    got = []
    for slot in (0, 1):
        keys = TK.ticket_keys([slot, slot], [b"name", b"name"], 0)
        a = np.zeros(256, dtype=np.uint8)
        a[0:4] = np.frombuffer(b"name", np.uint8)
        a[16:18] = np.frombuffer((16).to_bytes(2, "big"), np.uint8)
        d = np.zeros(1, dtype=TK.TICKET)
        d[0] = (0, 50, 16)
        ta = torch.from_numpy(a).to(DEV)
        res = torch.zeros(16, dtype=torch.uint8, device=DEV)
        try:
            TK.write(kt, keys, d, 1, ta, res)
            torch.cuda.synchronize()
            got.append((0, ta.cpu().numpy().tobytes(), res.cpu().numpy().tobytes()))
        except RuntimeError as e:
            got.append((str(e),))
    assert got[0] == got[1]
    assert got[0][0] != 0 or any(int(v) != 0 for v in np.frombuffer(got[0][2], dtype=TK.TICKET_RES)["status"])
    kt.close()


# ---- key expansion ----------------------------------------------------------------------------
@pytest.mark.parametrize("cipher,mac", A.SUITES)
def test_key_expansion_then_records(cipher, mac):
    """tlsrec_tls12_keytab_derive_cbc on 5 connections: records under the 10 derived slots match the model
    keyed from P_hash; tlsrec_tls12_make_keys_cbc gives the same material on the host"""
    hname, etm, count = ("sha384", 1, 5) if mac == R.MAC_SHA384 else ("sha256", 0, 5)
    prf = T.PRF_SHA384 if hname == "sha384" else T.PRF_SHA256
    kl, ml = A.KEYLEN[cipher], R.MACLEN[mac]
    raw = prng_bytes(800 + cipher, count * 112)
    conns = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(DEV)
    keys = []
    for i in range(count):
        master, rb = raw[112 * i:112 * i + 48], raw[112 * i + 48:112 * i + 112]
        blk = tls12_ref.p_hash(hname, master, b"key expansion" + rb, 2 * ml + 2 * kl)
        for side in (0, 1):
            keys.append(R.Key(cipher, mac, etm, blk[2 * ml + side * kl:2 * ml + (side + 1) * kl],
                              blk[side * ml:(side + 1) * ml]))
        if i == 0:
            st, cw, sw = C.make_keys(prf, cipher, mac, master, rb)
            assert st == 0
            assert bytes(cw["key"][0][:kl]) == keys[0].key and bytes(sw["mac_key"][0][:ml]) == keys[1].mac_key
            assert not any(cw["key"][0][kl:]) and not any(sw["mac_key"][0][ml:])
    kt = M.KeyTable(12)
    T.tls12_keytab_derive_cbc(kt, 1, count, cipher, mac, etm, prf, conns)
    torch.cuda.synchronize()
    slots = [None] + keys + [None]
    recs = [L.plain_rec(s, 7 * s, 90 + s, head=24) for s in range(12)]
    run = L.Run(slots, recs)
    want = run.expected(False)
    assert [w[0] for w in want].count(0) == 10
    out, res = run.gpu(False, kt=kt)
    bad = run.compare(False, out, res, True, want)
    assert not bad, bad[:5]
    back = L.Run(slots, _sealed(recs, want)[1:11])
    out, res = back.gpu(True, kt=kt)
    bad = back.compare(True, out, res)
    assert not bad, bad[:5]
    kt.close()


def test_key_expansion_error_order():
    lib, BAD, UNA = _abi.load(), M.ERR_SSL_BAD_INPUT_DATA, M.ERR_SSL_FEATURE_UNAVAILABLE
    kt = M.KeyTable(4)
    conns = torch.zeros(2 * 112, dtype=torch.uint8, device=DEV)
    f = lambda first, count, c, m, e, prf, p=conns.data_ptr(): lib.tlsrec_tls12_keytab_derive_cbc(
        kt.handle, first, count, c, m, e, prf, p, None)
    for c, m in A.SUITES:
        other = R.MAC_SHA1 if m != R.MAC_SHA1 else R.MAC_SHA256
        assert f(0, 3, c, other, 2, T.PRF_NONE) == BAD              # the range comes first
        assert f(0, 1, c, other, 2, T.PRF_NONE) == UNA              # then the pair
        assert f(0, 1, c, R.MAC_SHA1, 0, T.PRF_SHA256) == UNA       # a known MAC outside the pair
        assert f(0, 1, c, m, 2, T.PRF_NONE) == UNA                  # then the prf
        assert f(0, 1, c, m, 2, T.PRF_SHA256) == BAD                # then etm
        assert f(0, 0, c, m, 0, T.PRF_SHA256) == 0
    assert f(0, 1, 25, R.MAC_SHA256, 0, T.PRF_SHA256) == UNA
    kt.close()


# ---- the record server and the AEAD-only entry points that need a table ---------------------
def _record(n=40):
    from mbedtls_amd.record import Record
    return Record(ctr=bytes(8), type=23, ver=b"\x03\x03", buf=bytearray(prng_bytes(9, 16 + n) + bytes(64)),
                  data_offset=16, data_len=n)


def _refused_transform(cipher):
    """what tlsrec_transform_setup leaves of a transform it refuses"""
    from mbedtls_amd.record import Transform
    t = Transform.__new__(Transform)
    t._lib, t._t = _abi.load(), _abi.CTransform()
    r = t._lib.tlsrec_transform_setup(ctypes.byref(t._t), M.VERSION_TLS1_2, cipher, bytes(32), bytes(32), bytes(16),
                                      bytes(16))
    return r, t


def _served(t):
    """tlsrec_encrypt_buf and tlsrec_decrypt_buf through the record server: statuses, record fields, bytes"""
    out = []
    for fn in (t.encrypt_buf, t.decrypt_buf):
        rec = _record()
        st = fn(rec)
        out.append((st, rec.data_offset, rec.data_len, rec.type, bytes(rec.buf), rec.cid))
    return out


@pytest.mark.parametrize("cipher", sorted(A.KEYLEN))
def test_the_record_server_takes_no_transform_of_a_new_id(cipher):
    """tlsrec_transform_setup answers 26..29 as it answers an unknown cipher and allocates no slot; what it
    leaves is served by tlsrec_encrypt_buf / _decrypt_buf exactly as the unknown cipher's remains, and a
    transform without slots that names the id as one that names id 25"""
    from mbedtls_amd.record import Transform
    r, t = _refused_transform(cipher)
    r25, t25 = _refused_transform(25)
    assert r == r25 == M.ERR_SSL_FEATURE_UNAVAILABLE
    assert bytes(t._t) == bytes(t25._t) and (t._t.slot_enc, t._t.slot_dec) == (-1, -1)
    got, got25 = _served(t), _served(t25)
    assert got == got25
    assert all(g[0] != 0 for g in got)
    assert all(g[4] == bytes(_record().buf) for g in got)             # no byte of either record changed
    # the engine's own slot table refuses the key material too
    f = _abi.load().tlsrec__engine_slot_alloc
    f.argtypes, f.restype = [ctypes.c_void_p], ctypes.c_int
    km = M.key_material(M.CIPHER_AES_128_GCM, M.VERSION_TLS1_2, bytes(16), bytes(16))
    km25 = km.copy()
    km["cipher"], km25["cipher"] = cipher, 25
    a, b = f(km.ctypes.data), f(km25.ctypes.data)
    assert a == b and a < 0
    # an AES-GCM transform's fields with the id written in and no slots: as the same naming id 25
    pair = []
    for c in (cipher, 25):
        live = Transform(M.VERSION_TLS1_2, M.CIPHER_AES_128_GCM, bytes(16), bytes(16), bytes(16), bytes(16))
        keep = bytes(live._t)
        live.close()
        ghost = Transform.__new__(Transform)
        ghost._lib, ghost._t = _abi.load(), _abi.CTransform.from_buffer_copy(keep)
        ghost._t.cipher, ghost._t.slot_enc, ghost._t.slot_dec = c, -1, -1
        pair.append(_served(ghost))
        ghost._t = None
    assert pair[0] == pair[1] and all(g[0] != 0 for g in pair[0])
    t._t = t25._t = None


def test_aead_entry_points_with_a_table_answer_unknown_for_the_new_ids():
    """tlsrec_keytab_load, tlsrec_tls12_keytab_derive, tlsrec_tls13_keytab_derive: 26..29 as 25, nothing loaded"""
    lib, UNA = _abi.load(), M.ERR_SSL_FEATURE_UNAVAILABLE
    kt = M.KeyTable(4)
    conns = torch.zeros(2 * 112, dtype=torch.uint8, device=DEV)
    secrets = torch.zeros(4 * 64, dtype=torch.uint8, device=DEV)
    for c in sorted(A.KEYLEN) + [25]:
        km = M.key_material(M.CIPHER_AES_128_GCM, M.VERSION_TLS1_2, bytes(16), bytes(16))
        km["cipher"] = c
        assert lib.tlsrec_keytab_load(kt.handle, 0, 1, km.ctypes.data, 0, None) == UNA
        assert lib.tlsrec_tls12_keytab_derive(kt.handle, 0, 1, c, T.PRF_SHA256, conns.data_ptr(), None) == UNA
        assert lib.tlsrec_tls13_keytab_derive(kt.handle, 0, 1, c, secrets.data_ptr(), 0, None) == UNA
    torch.cuda.synchronize()
    recs = [L.plain_rec(s, 20, s) for s in range(4)]                  # every slot is still unloaded
    run = L.Run([None] * 4, recs)
    out, res = run.gpu(False, kt=kt)
    assert not run.compare(False, out, res)
    kt.close()


def test_one_load_call_of_mixed_kinds():
    """AES, ARIA, ARIA, AES, Camellia, AES in one tlsrec_keytab_load_cbc call (runs of one kind, each set up by
    its own kernel), host and device material: every slot works"""
    spec = [(R.CIPHER_AES_128_CBC, R.MAC_SHA1, 0), (ARIA128, R.MAC_SHA256, 1), (ARIA256, R.MAC_SHA384, 0),
            (R.CIPHER_AES_256_CBC, R.MAC_SHA384, 1), (CAM128, R.MAC_SHA256, 0), (R.CIPHER_AES_128_CBC, R.MAC_SHA256, 1)]
    slots = [L.make_key(900 + i, c, m, e) for i, (c, m, e) in enumerate(spec)]
    km = np.concatenate([C.key_material(s.cipher, s.mac, s.etm, s.key, s.mac_key) for s in slots])
    recs = [L.plain_rec(i % 6, 10 * i + 3, i, head=24) for i in range(18)]
    run = L.Run(slots, recs)
    want = run.expected(False)
    for on_device in (False, True):
        kt = M.KeyTable(6)
        C.load(kt, torch.from_numpy(km.view(np.uint8).copy()).to(DEV) if on_device else km)
        out, res = run.gpu(False, kt=kt)
        bad = run.compare(False, out, res, True, want)
        assert not bad, (on_device, bad[:5])
        back = L.Run(slots, _sealed(recs, want))
        out, res = back.gpu(True, kt=kt)
        bad = back.compare(True, out, res)
        assert not bad, (on_device, bad[:5])
        kt.close()
