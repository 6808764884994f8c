"""AES-CBC + HMAC batch records on the GPU, bit-exact against tests/cbc_ref.py
(the CBC branches of library/ssl_msg.c restated) and, for the AEAD records of a
mixed batch, against oracle/.  Every record of every batch is compared."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import mbedtls_amd as M
from mbedtls_amd import _abi
from mbedtls_amd import cbc as C
from tests import batchlib as B
from tests import cbc_ref as R
from tests import cbclib as L
from tests import tls12_ref
from tests.batchlib import launch_log  # noqa: F401  (fixture)
from tests.prng import prng_bytes

pytestmark = pytest.mark.gpu

# AES block edges and the SHA-256 / SHA-512 padding edges behind a 13-byte header
LENGTHS = [0, 1, 15, 16, 17, 42, 43, 51, 98, 99, 115, 1400, 16384]
MACS = [R.MAC_SHA1, R.MAC_SHA256, R.MAC_SHA384]


@pytest.mark.parametrize("inplace", [True, False])
def test_round_trip_and_known_answers(inplace):
    """2 ciphers x 3 MACs x 2 orders x 13 lengths: the wire bytes equal the
    model's, and decrypt back; out of place the IV is copied to the output"""
    slots = [L.make_key(100 + i, c, m, e) for i, (c, m, e) in enumerate(L.ALL_KEYS)]
    recs = [L.plain_rec(s, n, 1000 * s + n) for s in range(len(slots)) for n in LENGTHS]
    run = L.Run(slots, recs)
    kt = L.load_table(slots)
    want = run.expected(False)
    assert all(w[0] == 0 for w in want)
    out, res = run.gpu(False, inplace=inplace, kt=kt)
    assert not run.compare(False, out, res, inplace, want), run.compare(False, out, res, inplace, want)[:5]
    sealed = [B.Rec(r.slot, bytearray(w[5]), w[1], w[2], r.ctr, w[3], r.ver) for r, w in zip(recs, want)]
    back = L.Run(slots, sealed)
    out, res = back.gpu(True, inplace=inplace, kt=kt)
    bad = back.compare(True, out, res, inplace)
    assert not bad, bad[:5]
    for i, (r, s) in enumerate(zip(recs, sealed)):          # and it is the plaintext we started from
        o = back.offs[i] + int(res[i]["data_offset"])
        assert int(res[i]["data_len"]) == r.data_len
        assert bytes(out[o:o + r.data_len]) == bytes(r.buf[r.data_offset:r.data_offset + r.data_len])
    kt.close()


def _pre_record(key, plaintext_len, padlen):
    """IV || plaintext || MAC || padding before encryption (the reference test's rec_save)"""
    ctr, ver = bytes(8), b"\x03\x03"
    data = bytes([42]) * plaintext_len
    mac = R._mac(key, ctr, 23, ver, data, b"")
    return bytes([0x55]) * 16 + data + mac + bytes([padlen]) * (padlen + 1)


def _seal(key, pre):
    return pre[:16] + R.aes_cbc(key.key, pre[:16], pre[16:], True)


@pytest.mark.parametrize("mac", MACS)
def test_padding_and_mac_sweep(mac):
    """ssl_decrypt_non_etm_cbc (tests/suites/test_suite_ssl_decrypt.function:125-313)
    as one batch per MAC: flip each byte, wrong padding values"""
    key = L.make_key(7, R.CIPHER_AES_128_CBC, mac, 0)
    maclen = R.MACLEN[mac]
    cases = []                                   # (pre-encryption record, expected status)

    def shape(sel):
        if sel < 0:
            padlen = 16 - (maclen + 1) % 16
            if sel == -2:
                padlen += 16 * ((255 - padlen) // 16)
            return 0, padlen
        return 16 - (sel + maclen + 1) % 16, sel

    for sel in (-1, -2, 0, 1, 15, 16, 17, 240, 255):            # the flip-each-byte loop
        pl, padlen = shape(sel)
        pre = _pre_record(key, pl, padlen)
        cases.append((pre, 0))
        for i in range(16, len(pre)):
            b = bytearray(pre)
            b[i] ^= 1
            cases.append((bytes(b), M.ERR_SSL_INVALID_MAC))
    for sel in range(256):                                      # the pad-value loop
        pl, padlen = shape(sel)
        pre = _pre_record(key, pl, padlen)
        values = range(padlen, 256) if sel in (0, 1, 239, 254) else sorted({padlen, min(padlen + 1, 255), 255})
        for v in values:
            b = bytearray(pre)
            b[len(b) - padlen - 1:] = bytes([v]) * (padlen + 1)
            cases.append((bytes(b), 0 if v == padlen else M.ERR_SSL_INVALID_MAC))
    recs = [B.Rec(0, bytearray(_seal(key, pre)), 0, len(pre), bytes(8), 23) for pre, _ in cases]
    run = L.Run([key], recs)
    want = run.expected(True)
    assert [w[0] for w in want] == [st for _, st in cases]      # the model agrees with the construction
    out, res = run.gpu(True)
    bad = run.compare(True, out, res, True, want)
    assert not bad, (len(bad), bad[:5])


@pytest.mark.parametrize("etm", [0, 1])
def test_length_checks(etm):
    """data_len below 32, below 16 + maclen + 1, not a multiple of 16 (for
    encrypt-then-MAC after the MAC is removed): all INVALID_MAC"""
    slots = [L.make_key(20 + m, R.CIPHER_AES_256_CBC, m, etm) for m in MACS]
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
    out, res = run.gpu(True)
    bad = run.compare(True, out, res, True, want)
    assert not bad, bad[:5]


def test_little_space_on_encrypt():
    """ssl_crypt_record_small: BUFFER_TOO_SMALL at ssl_msg.c:909, :1098, :1116 and
    :1199 -- every buffer length from none to ample, and short heads"""
    slots = [L.make_key(40 + i, R.CIPHER_AES_128_CBC, m, e) for i, (m, e) in
             enumerate((m, e) for m in MACS for e in (0, 1))]
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
    # the largest buffer that fails is followed by the smallest that passes
    assert any(a == M.ERR_SSL_BUFFER_TOO_SMALL and b == 0 for a, b in zip(st, st[1:]))
    out, res = run.gpu(False)
    bad = run.compare(False, out, res, True, want)
    assert not bad, bad[:5]


def test_encrypt_then_mac_tampering():
    """a flipped IV, ciphertext or MAC byte: INVALID_MAC with the reference's
    fields, and nothing outside the record buffer written"""
    slots = [L.make_key(60 + m, R.CIPHER_AES_128_CBC, m, 1) for m in MACS]
    recs = []
    for s, k in enumerate(slots):
        good = L.sealed_rec(k, s, 100, 70 + s)
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
    """epoch + 48-bit sequence in ctr, version FE FD; CID slots wrap the content
    in a DTLSInnerPlaintext; a wrong CID is UNEXPECTED_CID, an all-zero inner
    plaintext INVALID_RECORD"""
    ver = b"\xfe\xfd"
    cid = bytes(range(0x10, 0x15))
    keys = [(R.CIPHER_AES_128_CBC, R.MAC_SHA256, 0), (R.CIPHER_AES_256_CBC, R.MAC_SHA384, 1),
            (R.CIPHER_AES_128_CBC, R.MAC_SHA1, 1), (R.CIPHER_AES_256_CBC, R.MAC_SHA256, 0)]
    slots = [L.make_key(80 + i, c, m, e, cid=(cid if i % 2 == 0 else b"") if i < 3 else bytes(range(32)))
             for i, (c, m, e) in enumerate(keys)]
    ctr = lambda i: (1).to_bytes(2, "big") + (1000 + i).to_bytes(6, "big")
    plain = [L.plain_rec(s, n, 3 * s + n, tail=128, ver=ver, ctr=ctr(n)) for s in range(len(slots))
             for n in (0, 1, 15, 16, 100, 1400)]
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
    # an inner plaintext of zeros only, sealed by hand under slot 0
    k0 = slots[0]
    zero = bytearray(L.plain_rec(0, 0, 5, tail=128, ver=ver, ctr=ctr(7)).buf)
    inner = bytes(16)
    mac = R._mac(k0, ctr(7), M.MSG_CID, ver, inner, cid)
    body = inner + mac
    padlen = 15 - len(body) % 16
    body += bytes([padlen]) * (padlen + 1)
    zero[16:16 + len(body)] = R.aes_cbc(k0.key, bytes(zero[:16]), body, True)
    sealed.append(B.Rec(0, zero, 0, 16 + len(body), ctr(7), M.MSG_CID, ver, cid))
    back = L.Run(slots, sealed)
    want = back.expected(True)
    assert [w[0] for w in want[-4:]] == [M.ERR_SSL_UNEXPECTED_CID] * 3 + [M.ERR_SSL_INVALID_RECORD]
    out, res = back.gpu(True)
    bad = back.compare(True, out, res, True, want)
    assert not bad, bad[:5]


def test_one_shuffled_batch_of_aead_and_cbc(launch_log):  # noqa: F811
    """AES-128-GCM, ChaCha20-Poly1305, AES-128-CCM and every CBC variant in one
    batch, one record naming an unloaded slot; each kernel family ran"""
    aead = B.random_slots(5, [M.CIPHER_AES_128_GCM, M.CIPHER_CHACHA20_POLY1305, M.CIPHER_AES_128_CCM],
                          [M.VERSION_TLS1_2], 3)
    slots = list(aead) + [None] + [L.make_key(200 + i, c, m, e) for i, (c, m, e) in enumerate(L.ALL_KEYS)]
    order = np.random.default_rng(11).permutation(len(slots) * 6)
    recs = [L.plain_rec(int(j) % len(slots), [0, 17, 100, 1400, 333, 16][int(j) // len(slots)], int(j), head=24)
            for j in order]
    run = L.Run(slots, recs)
    want = run.expected(False)
    assert [w[0] for w in want].count(M.ERR_SSL_BAD_INPUT_DATA) == 6
    kt = L.load_table(slots)
    out, res = run.gpu(False, kt=kt)
    bad = run.compare(False, out, res, True, want)
    assert not bad, bad[:5]
    kinds = {e[0] for e in launch_log()}
    assert {_abi.LOG_CBC, _abi.LOG_GCM, _abi.LOG_CHACHA, _abi.LOG_CCM} <= kinds
    assert launch_log(_abi.LOG_BUCKET)[-1][1] == 1
    cbc = launch_log(_abi.LOG_CBC)[-1]
    assert cbc[1:4] == (0, 0b1110, 0b11)          # encrypt, all three MACs, both orders
    sealed = [B.Rec(r.slot, bytearray(w[5]), w[1], w[2], r.ctr, w[3], r.ver) for r, w in zip(recs, want)]
    back = L.Run(slots, sealed)
    out, res = back.gpu(True, kt=kt)
    bad = back.compare(True, out, res, True)
    assert not bad, bad[:5]
    assert launch_log(_abi.LOG_CBC)[-1][1] == 1
    kt.close()


def test_slot_reload_cbc_aead_cbc():
    k1 = L.make_key(300, R.CIPHER_AES_256_CBC, R.MAC_SHA384, 0)
    a = B.random_slots(9, [M.CIPHER_AES_256_GCM], [M.VERSION_TLS1_3], 1)[0]
    k2 = L.make_key(301, R.CIPHER_AES_128_CBC, R.MAC_SHA1, 1)
    other = L.make_key(302, R.CIPHER_AES_128_CBC, R.MAC_SHA256, 0)
    kt = L.load_table([k1, other])
    for s in (k1, a, k2):
        if isinstance(s, R.Key):
            C.load(kt, C.key_material(s.cipher, s.mac, s.etm, s.key, s.mac_key), first=0)
        else:
            kt.load(M.key_material(*a), first=0)
        recs = [L.plain_rec(i % 2, n, n, head=24) for i, n in enumerate((0, 1, 100, 101, 1400, 1401))]
        run = L.Run([s, other], recs)
        out, res = run.gpu(False, kt=kt)
        bad = run.compare(False, out, res)
        assert not bad, (type(s), bad[:5])
    kt.close()


def test_unreached_cbc_record_fails_closed():
    """the skip-record hook on a CBC record leaves INTERNAL_ERROR"""
    with _abi.use_library() as lib:
        f = lib.tlsrec__test_skip_record
        f.argtypes, f.restype = [ctypes.c_uint32], None
        try:
            for slots in ([L.make_key(400, R.CIPHER_AES_128_CBC, R.MAC_SHA256, 0)],
                          [L.make_key(401 + i, c, m, e) for i, (c, m, e) in enumerate(L.ALL_KEYS[:4])]):
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
    slots = [L.make_key(500 + i, c, m, e) for i, (c, m, e) in enumerate(L.ALL_KEYS[::3])]
    recs = [L.plain_rec(i % len(slots), n, 40 + i) for i, n in enumerate((0, 16, 100, 1400, 4000, 17, 333, 15))]
    run = L.Run(slots, recs)
    want = run.expected(False)
    kt = L.load_table(slots)
    out, res = run.gpu(False, kt=kt, host=True)
    bad = run.compare(False, out, res, True, want)
    assert not bad, bad[:5]
    sealed = [B.Rec(r.slot, bytearray(w[5]), w[1], w[2], r.ctr, w[3], r.ver) for r, w in zip(recs, want)]
    back = L.Run(slots, sealed)
    out, res = back.gpu(True, kt=kt, host=True)
    bad = back.compare(True, out, res)
    assert not bad, bad[:5]
    kt.close()


@pytest.mark.parametrize("prf,hname", [(M.tls12.PRF_SHA256, "sha256"), (M.tls12.PRF_SHA384, "sha384")])
def test_key_expansion_then_records(prf, hname):
    """tlsrec_tls12_make_keys_cbc against P_hash + a slice by hand, then client
    encrypts, server decrypts"""
    master, rb = prng_bytes(1, 48), prng_bytes(2, 64)
    cipher, mac = (R.CIPHER_AES_256_CBC, R.MAC_SHA384) if hname == "sha384" else (R.CIPHER_AES_128_CBC, R.MAC_SHA256)
    kl, ml = R.KEYLEN[cipher], R.MACLEN[mac]
    blk = tls12_ref.p_hash(hname, master, b"key expansion" + rb, 2 * ml + 2 * kl)
    st, cw, sw = C.make_keys(prf, cipher, mac, master, rb)
    assert st == 0
    for i, d in enumerate((cw, sw)):
        assert bytes(d["mac_key"][0][:ml]) == blk[i * ml:(i + 1) * ml] and not any(d["mac_key"][0][ml:])
        assert bytes(d["key"][0][:kl]) == blk[2 * ml + i * kl:2 * ml + (i + 1) * kl] and not any(d["key"][0][kl:])
        assert (int(d["cipher"][0]), int(d["tls_minor"][0]), int(d["mac"][0]), int(d["etm"][0])) == (cipher, 3, mac, 0)
    client, server = M.KeyTable(1), M.KeyTable(1)
    C.load(client, cw)
    C.load(server, cw)           # the server reads what the client writes: client_write material
    key = R.Key(cipher, mac, 0, bytes(cw["key"][0][:kl]), bytes(cw["mac_key"][0][:ml]))
    recs = [L.plain_rec(0, n, n) for n in (0, 1, 100, 1400)]
    run = L.Run([key], recs)
    want = run.expected(False)
    out, res = run.gpu(False, kt=client)
    assert not run.compare(False, out, res, True, want)
    sealed = [B.Rec(0, bytearray(out[o:o + len(r.buf)]), int(g["data_offset"]), int(g["data_len"]), r.ctr, 23)
              for r, o, g in zip(recs, run.offs, res)]
    back = L.Run([key], sealed)
    out, res = back.gpu(True, kt=server)
    assert not back.compare(True, out, res)
    assert [int(g["data_len"]) for g in res] == [0, 1, 100, 1400]
    client.close()
    server.close()


# ---- out of scope for the framing layers, tickets: a CBC slot is a never-loaded slot ----
_AEAD = (M.CIPHER_AES_128_GCM, M.VERSION_TLS1_2, bytes(16), bytes(16), 0)


def _cbc_and_empty_table():
    """slot 0 holds a CBC key, slot 1 was never loaded"""
    key = L.make_key(600, R.CIPHER_AES_128_CBC, R.MAC_SHA256, 0)
    return L.load_table([key, None]), key


def _sealed_body(key, ctr, ver, n=100, seed=1):
    r = L.sealed_rec(key, 0, n, seed, ver=ver, ctr=ctr)
    return bytes(r.buf[r.data_offset:r.data_offset + r.data_len])


def _same(a, b, skip=()):
    """two structured records equal in every field but `skip`"""
    return all(np.array_equal(a[f], b[f]) for f in a.dtype.names if f not in skip)


def test_stream_calls_treat_a_cbc_slot_as_unloaded():
    kt, key = _cbc_and_empty_table()
    c = B.Conns.__new__(B.Conns)
    c.slots, c.kt, c.ot = [_AEAD, _AEAD], kt, []
    data = prng_bytes(3, 3000)
    (s0, o0), (s1, o1) = c.encrypt([(0, data, 5, 1000, 23), (1, data, 5, 1000, 23)])
    assert _same(s0, s1, skip=("first",)) and o0 == o1 and c.last_regions[0] == c.last_regions[1]
    assert int(s0["status"]) != 0
    # receive: two well-formed records the CBC key would open
    wire = b""
    for seq in (7, 8):
        body = _sealed_body(key, seq.to_bytes(8, "big"), b"\x03\x03", seed=seq)
        wire += bytes([23, 3, 3]) + len(body).to_bytes(2, "big") + body
    a, recs, res, sres, offs = c.decrypt([(0, wire, 7, 0), (1, wire, 7, 0)])
    assert _same(sres[0], sres[1], skip=("first",)), (sres[0], sres[1])
    assert int(sres[0]["status"]) != 0 and int(sres[0]["nrec"]) == 0
    f0, f1, n = int(sres[0]["first"]), int(sres[1]["first"]), int(sres[0]["nparsed"])
    for k in range(n):
        assert _same(res[f0 + k], res[f1 + k]), (k, res[f0 + k], res[f1 + k])
        assert int(res[f0 + k]["status"]) != 0
    assert bytes(a[offs[0]:offs[0] + len(wire)]) == bytes(a[offs[1]:offs[1] + len(wire)])
    kt.close()


def test_dtls_calls_treat_a_cbc_slot_as_unloaded():
    kt, key = _cbc_and_empty_table()
    t = B.Table.__new__(B.Table)
    t.slots, t.gran_of, t.kt, t.ot = [(M.CIPHER_AES_128_GCM, bytes(16), bytes(16), b"")] * 2, {}, kt, []
    ctr = (1).to_bytes(2, "big") + (9).to_bytes(6, "big")
    data = prng_bytes(4, 2500)
    (s0, o0, _, _), (s1, o1, _, _) = t.encrypt([(0, data, ctr, 1000, 23), (1, data, ctr, 1000, 23)])
    assert _same(s0, s1, skip=("first",)) and o0 == o1 and t.last_regions[0] == t.last_regions[1]
    assert int(s0["status"]) == M.ERR_SSL_BAD_INPUT_DATA
    body = _sealed_body(key, ctr, b"\xfe\xfd")
    dg = bytes([23, 0xfe, 0xfd]) + ctr + len(body).to_bytes(2, "big") + body
    a, recs, res, disp, cres, offs = t.decrypt([(0, {"in_epoch": 1}, [dg, dg]), (1, {"in_epoch": 1}, [dg, dg])])
    assert _same(cres[0], cres[1], skip=("first",)), (cres[0], cres[1])
    assert int(cres[0]["status"]) == M.ERR_SSL_BAD_INPUT_DATA and int(cres[0]["naccepted"]) == 0
    f0, f1 = int(cres[0]["first"]), int(cres[1]["first"])
    for k in range(int(cres[0]["nrec"])):
        assert _same(res[f0 + k], res[f1 + k]) and disp[f0 + k] == disp[f1 + k]
    for p0, p1 in zip(offs[0], offs[1]):
        assert bytes(a[p0:p0 + len(dg)]) == bytes(a[p1:p1 + len(dg)])
    kt.close()


def test_ticket_calls_treat_a_cbc_slot_as_unloaded():
    import torch
    from mbedtls_amd import ticket as T
    kt, _ = _cbc_and_empty_table()
    dev = torch.device("cuda")
    states = [prng_bytes(50 + i, n) for i, n in enumerate((0, 16, 100))]
    got = []
    for slot in (0, 1):
        keys = T.ticket_keys([slot, slot], [b"name", b"name"], 0)
        per = []
        for fn in (T.write, T.parse):
            a = np.zeros(len(states) * 256, dtype=np.uint8)
            d = np.zeros(len(states), dtype=T.TICKET)
            for i, st in enumerate(states):
                o = 256 * i
                a[o:o + 4] = np.frombuffer(b"name", np.uint8)
                a[o + 4:o + 16] = 7
                a[o + 16:o + 18] = np.frombuffer(len(st).to_bytes(2, "big"), np.uint8)
                a[o + 18:o + 18 + len(st)] = np.frombuffer(st, np.uint8)
                d[i] = (o, 34 + len(st), len(st)) if fn is T.write else (o, 34 + len(st), 0)
            ta = torch.from_numpy(a).to(dev)
            res = torch.zeros(len(states) * 16, dtype=torch.uint8, device=dev)
            try:
                fn(kt, keys, d, len(states), ta, res)
                torch.cuda.synchronize()
                per.append((0, ta.cpu().numpy().tobytes(), res.cpu().numpy().tobytes()))
            except RuntimeError as e:
                per.append((str(e),))
        got.append(per)
    assert got[0] == got[1]
    for x in got[0]:                      # and it is a refusal, whichever form it takes
        assert x[0] != 0 or any(int(v) != 0 for v in np.frombuffer(x[2], dtype=T.TICKET_RES)["status"])
    kt.close()
