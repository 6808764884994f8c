"""Batch key derivation for the AES-CBC + HMAC suites on the GPU
(tlsrec_tls12_keytab_derive_cbc): device connections -> P_hash -> the CBC split
of the key block -> key-table slots, checked through what the slots then do.
Expected keys come from P_hash over hashlib (cross-checked by OpenSSL's
TLS1-PRF), expected records from the CBC record model of tests/cbc_ref.py (the
AEAD ones from oracle/), expected streams and datagrams from the framing model
of tests/cbc_frames_ref.py.  Everything is bit-exact."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

import mbedtls_amd as M  # noqa: E402
from mbedtls_amd import cbc as C  # noqa: E402
from mbedtls_amd import tls12 as T  # noqa: E402
from tests import batchlib as B  # noqa: E402
from tests import cbc_frames_ref as F  # noqa: E402
from tests import cbc_ref as R  # noqa: E402
from tests import cbclib as CL  # noqa: E402
from tests import test_cbc_frames_gpu as FG  # noqa: E402  (its send / receive harness)
from tests.prng import prng_bytes  # noqa: E402
from tests.tls12_ref import evp_tls1_prf, p_hash, split_key_block  # noqa: E402

DEV = torch.device("cuda")
PRF = {"sha256": T.PRF_SHA256, "sha384": T.PRF_SHA384}
A128, A256 = R.CIPHER_AES_128_CBC, R.CIPHER_AES_256_CBC
BAD, UNA = M.ERR_SSL_BAD_INPUT_DATA, M.ERR_SSL_FEATURE_UNAVAILABLE
# every (cipher, mac, prf); etm alternates over the cases, so each (cipher, mac) sees both orders
COMBOS = [(c, m, h, k % 2) for k, (c, m, h) in
          enumerate(itertools.product((A128, A256), (R.MAC_SHA1, R.MAC_SHA256, R.MAC_SHA384), ("sha256", "sha384")))]
assert all({e for c, m, h, e in COMBOS if m == mac} == {0, 1} for mac in (1, 2, 3))


def _conns(seed, count, unaligned=False):
    raw = prng_bytes(seed, count * 112)
    buf = torch.zeros(count * 112 + 16, dtype=torch.uint8, device=DEV)
    off = 1 if unaligned else 0
    conns = buf[off:off + count * 112]
    conns.copy_(torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()))
    assert (conns.data_ptr() % 16 != 0) == unaligned
    return raw, conns


def _key_block(hname, master, rb, n):
    want = p_hash(hname, master, b"key expansion" + rb, n)
    try:
        other = evp_tls1_prf(hname, master, b"key expansion" + rb, n)
    except (OSError, AttributeError):       # no OpenSSL 3 on this machine: hashlib alone
        other = want
    assert other == want
    return want


def _expected_keys(hname, cipher, mac, etm, raw, count, cids=None):
    """tests/cbc_ref.Key of the 2 * count slots: client_write, server_write per connection
    (ssl_tls.c:7858-7886: client_mac | server_mac | client_key | server_key)"""
    kl, ml = R.KEYLEN[cipher], R.MACLEN[mac]
    keys = []
    for i in range(count):
        master, rb = raw[112 * i:112 * i + 48], raw[112 * i + 48:112 * i + 112]
        blk = _key_block(hname, master, rb, 2 * ml + 2 * kl)
        for side in (0, 1):
            keys.append(R.Key(cipher, mac, etm, blk[2 * ml + side * kl:2 * ml + (side + 1) * kl],
                              blk[side * ml:(side + 1) * ml], (cids or {}).get(2 * i + side, b"")))
    return keys


def _derive(kt, first, count, cipher, mac, etm, hname, conns, raw):
    T.tls12_keytab_derive_cbc(kt, first, count, cipher, mac, etm, PRF[hname], conns)
    torch.cuda.synchronize()
    assert conns.cpu().numpy().tobytes() == raw, "conns is only read"


def _check_records(kt, slots, lengths, seed, unloaded=(), ver=b"\x03\x03"):
    """One batch encrypts a record per loaded slot of `slots` (Key / batchlib tuple / None) plus one per slot
    id of `unloaded`, a second decrypts model-sealed records: status, data_offset, data_len, type and bytes
    against the model; the records naming an unloaded slot come back BAD_INPUT_DATA, buffers untouched."""
    live = [s for s, k in enumerate(slots) if k is not None]
    assert len(lengths) == len(live)
    ctr = lambda j: (1).to_bytes(2, "big") + (40 + j).to_bytes(6, "big")
    plain = [CL.plain_rec(s, n, seed + 7 * j, head=24, tail=128, ver=ver, ctr=ctr(j))
             for j, (s, n) in enumerate(zip(live, lengths))]
    extra = [CL.plain_rec(s, 40 + 3 * j, seed + 1000 + j, ver=ver) for j, s in enumerate(unloaded)]
    recs = extra[:len(extra) // 2] + plain + extra[len(extra) // 2:]
    run = CL.Run(slots, recs)
    want = run.expected(False)
    assert [w[0] for w in want].count(BAD) == len(extra) and [w[0] for w in want].count(0) == len(plain)
    out, res = run.gpu(False, kt=kt)
    bad = run.compare(False, out, res, True, want)
    assert not bad, bad[:5]
    for i, r in enumerate(recs):
        if want[i][0] == BAD:
            assert bytes(out[run.offs[i]:run.offs[i] + len(r.buf)]) == bytes(r.buf), (i, r.slot)
    if all(isinstance(slots[s], R.Key) for s in live):
        sealed = [CL.sealed_rec(slots[s], s, n, seed + 7 * j, head=24, tail=128, ver=ver, ctr=ctr(j))
                  for j, (s, n) in enumerate(zip(live, lengths))]
    else:                                   # AEAD slots: the batch's own output, opened again
        sealed = [B.Rec(r.slot, bytearray(w[5]), w[1], w[2], r.ctr, w[3], r.ver) for r, w in zip(recs, want)
                  if w[0] == 0]
    back = CL.Run(slots, sealed)
    want = back.expected(True)
    assert all(w[0] == 0 for w in want) and [w[2] for w in want] == list(lengths)
    out, res = back.gpu(True, kt=kt)
    bad = back.compare(True, out, res, True, want)
    assert not bad, bad[:5]


@pytest.mark.parametrize("cipher,mac,hname,etm", COMBOS)
def test_every_combination(cipher, mac, hname, etm):
    count, first = 65, 3
    raw, conns = _conns(0xCB00 + 16 * cipher + 4 * mac + (hname == "sha384"), count)
    kt = M.KeyTable(first + 2 * count + 2)
    _derive(kt, first, count, cipher, mac, etm, hname, conns, raw)
    slots = [None] * first + _expected_keys(hname, cipher, mac, etm, raw, count) + [None] * 2
    lengths = [(37 * k) % 300 for k in range(2 * count)]
    assert 0 in lengths
    _check_records(kt, slots, lengths, seed=91, unloaded=[0, 1, 2, first + 2 * count, first + 2 * count + 1])
    kt.close()


# the longest chain (4 P_SHA384 iterations), and the one shape whose key offsets are no multiple of 16 bytes
EDGE_SHAPES = [(A256, R.MAC_SHA384, "sha384", 0), (A128, R.MAC_SHA1, "sha256", 1)]


@pytest.mark.parametrize("cipher,mac,hname,etm", EDGE_SHAPES, ids=["aes256-sha384-prf384", "aes128-sha1-prf256"])
@pytest.mark.parametrize("count,unaligned", [(1, False), (63, False), (64, False), (65, False), (65, True)])
def test_workgroup_edges(cipher, mac, hname, etm, count, unaligned):
    """one lane per connection, 64 per workgroup; an array that is not 16-byte aligned takes the byte loads"""
    raw, conns = _conns(0xED00 + count + 256 * mac, count, unaligned)
    kt = M.KeyTable(2 * count)
    _derive(kt, 0, count, cipher, mac, etm, hname, conns, raw)
    _check_records(kt, _expected_keys(hname, cipher, mac, etm, raw, count),
                   [(37 * k) % 300 for k in range(2 * count)], seed=17)
    kt.close()


@pytest.mark.parametrize("cipher,mac,hname,etm", [(A128, R.MAC_SHA1, "sha256", 0), (A256, R.MAC_SHA384, "sha384", 1),
                                                  (A256, R.MAC_SHA256, "sha256", 1)])
def test_same_keys_as_the_host_path(cipher, mac, hname, etm):
    """tlsrec_tls12_make_keys_cbc + tlsrec_keytab_load_cbc and the batch derivation fill a table alike:
    the same records under the same IVs give the same bytes"""
    count = 5
    raw, conns = _conns(0x5A5A + mac, count)
    host, dev = M.KeyTable(2 * count), M.KeyTable(2 * count)
    for i in range(count):
        st, cw, sw = C.make_keys(PRF[hname], cipher, mac, raw[112 * i:112 * i + 48], raw[112 * i + 48:112 * i + 112])
        assert st == 0
        for side, km in enumerate((cw, sw)):
            km["etm"] = etm
            C.load(host, km, first=2 * i + side)
    _derive(dev, 0, count, cipher, mac, etm, hname, conns, raw)
    recs = [CL.plain_rec(s, (53 * s) % 200, 300 + s) for s in range(2 * count)]
    run = CL.Run([None] * (2 * count), recs)
    (out_h, res_h), (out_d, res_d) = run.gpu(False, kt=host), run.gpu(False, kt=dev)
    assert [int(x) for x in res_h["status"]] == [0] * len(recs)
    assert res_h.tobytes() == res_d.tobytes() and out_h.tobytes() == out_d.tobytes()
    assert out_h.tobytes() != run.arena.tobytes()
    host.close()
    dev.close()


def _aead_slots(hname, cipher, raw, count):
    """batchlib slot tuples the AEAD batch derivation leaves (tests/test_tls12_keys_gpu.py)"""
    kl, il = M.KEYLEN[cipher], 4
    slots = []
    for i in range(count):
        blk = p_hash(hname, raw[112 * i:112 * i + 48], b"key expansion" + raw[112 * i + 48:112 * i + 112],
                     2 * kl + 2 * il)
        ck, civ, sk, siv = split_key_block(blk, kl, il)
        slots += [(cipher, M.VERSION_TLS1_2, ck, civ + bytes(16 - il), 0),
                  (cipher, M.VERSION_TLS1_2, sk, siv + bytes(16 - il), 0)]
    return slots


def test_reload_in_both_directions():
    """AES-128-GCM slots -> CBC slots -> AES-128-GCM slots, each by its batch derivation; a connection ID set
    on a slot is gone after either derivation; a record sealed for the CBC key fails under the AEAD key as
    the oracle's AEAD decrypt says"""
    count, gcm = 6, M.CIPHER_AES_128_GCM
    cid = bytes(range(0x30, 0x38))
    dver = b"\xfe\xfd"
    raw1, conns1 = _conns(0x7E10, count)
    raw2, conns2 = _conns(0x7E11, count)
    raw3, conns3 = _conns(0x7E12, count)
    kt = M.KeyTable(2 * count)
    lengths = [(37 * k) % 300 for k in range(2 * count)]
    T.tls12_keytab_derive(kt, 0, count, gcm, T.PRF_SHA256, conns1)
    kt.set_cid(4, cid)
    _derive(kt, 0, count, A256, R.MAC_SHA384, 1, "sha384", conns2, raw2)
    keys = _expected_keys("sha384", A256, R.MAC_SHA384, 1, raw2, count)      # no Key carries a CID
    _check_records(kt, keys, lengths, seed=5)
    _check_records(kt, keys, lengths, seed=6, ver=dver)                       # slot 4: sealed without a CID
    kt.set_cid(5, cid)
    T.tls12_keytab_derive(kt, 0, count, gcm, T.PRF_SHA256, conns3)
    torch.cuda.synchronize()
    aead = _aead_slots("sha256", gcm, raw3, count)
    _check_records(kt, aead, lengths, seed=7)
    _check_records(kt, aead, lengths, seed=8, ver=dver)                       # slot 5: the same
    old = [CL.sealed_rec(keys[s], s, 100 + s, 900 + s) for s in range(2 * count)]
    run = CL.Run(aead, old)
    want = run.expected(True)
    assert all(w[0] == M.ERR_SSL_INVALID_MAC for w in want)
    out, res = run.gpu(True, kt=kt)
    bad = run.compare(True, out, res, True, want)
    assert not bad, bad[:5]
    kt.close()


def _framed_table(cipher, mac, etm, hname, seed, cid=b""):
    """3 connections derived into slots 1 .. 6; the model's slot list (client_write slots carry `cid`)"""
    count, first = 3, 1
    raw, conns = _conns(seed, count)
    kt = M.KeyTable(first + 2 * count)
    _derive(kt, first, count, cipher, mac, etm, hname, conns, raw)
    cw = [first + 2 * i for i in range(count)]
    for s in cw:
        if cid:
            kt.set_cid(s, cid)
    keys = _expected_keys(hname, cipher, mac, etm, raw, count, cids={2 * i: cid for i in range(count)})
    return kt, [None] * first + keys, cw


def test_through_the_stream_layer():
    """tlsrec_stream_encrypt_ex / _decrypt_ex with TLSREC_FRAME_CBC over a derived table: each connection's
    client_write slot sends two records (100 and 1 bytes) and the same slot receives them"""
    kt, slots, cw = _framed_table(A128, R.MAC_SHA256, 1, "sha256", 0xF4A0)
    jobs = [(s, prng_bytes(0x600 + s, 101), (1000 * s + 7).to_bytes(8, "big"), 100, 23) for s in cw]
    g = FG.send(kt, slots, jobs, False)
    FG.check_send(slots, g, False)
    assert [(int(r["status"]), int(r["nrec"])) for r in g["sres"]] == [(0, 2)] * 3
    conns = [(s, FG.wire_of(g, i), int.from_bytes(c8, "big"), 0) for i, (s, _, c8, _, _) in enumerate(jobs)]
    want = [F.stream_decrypt(FG.protector(slots[s]), data, c0.to_bytes(8, "big"), nbz) for s, data, c0, nbz in conns]
    assert [(w[0]["status"], w[0]["nrec"], [r[2] for r in w[1]]) for w in want] == [(0, 2, [100, 1])] * 3
    FG.check_stream(conns, want, FG.recv_stream(kt, conns))
    kt.close()


def test_through_the_dtls_layer_with_a_connection_id():
    """the same through tlsrec_dtls_encrypt_ex / _decrypt_ex, the slots given an 8-byte CID after the derive"""
    cid = bytes(range(0xC0, 0xC8))
    kt, slots, cw = _framed_table(A256, R.MAC_SHA384, 0, "sha384", 0xF4A1, cid)
    jobs = [(s, prng_bytes(0x700 + s, 101), FG.ctr(1, 50 * s), 100, 23) for s in cw]
    g = FG.send(kt, slots, jobs, True)
    FG.check_send(slots, g, True)
    assert [(int(r["status"]), int(r["nrec"])) for r in g["sres"]] == [(0, 2)] * 3
    hdr, conns = 13 + len(cid), []
    for i, (s, _, _, _, _) in enumerate(jobs):
        grams = []
        for k in range(2):
            j = g["firsts"][i] + k
            o = int(g["recs"][j]["buf_off"]) - hdr
            grams.append(g["out"][o:o + hdr + int(g["res"][j]["data_len"])].tobytes())
            assert grams[-1][0] == M.MSG_CID and grams[-1][11:11 + len(cid)] == cid
        conns.append((s, {"in_epoch": 1, "cid_len": len(cid)}, grams))
    want = []
    for s, stt, grams in conns:
        st = F.DtlsState(anti_replay=1, in_epoch=1, cid_len=len(cid))
        want.append((F.dtls_decrypt(FG.protector(slots[s]), st, grams), st))
    assert [(w[0]["status"], w[0]["naccepted"], [r[3] for r in w[1]]) for w, _ in want] == [(0, 2, [100, 1])] * 3
    FG.check_dtls(conns, want, FG.recv_dtls(kt, conns))
    kt.close()


def test_argument_checks():
    """every error of the call, in its order: the table, conns and the slot range; the cipher and the mac;
    the prf; etm"""
    fn = M.load().tlsrec_tls12_keytab_derive_cbc
    raw, conns = _conns(1, 4)
    p = conns.data_ptr()
    kt = M.KeyTable(9)                      # odd capacity: slots 0..8
    h = kt.handle
    ok = (A128, R.MAC_SHA256, 0, T.PRF_SHA256)
    # BAD_INPUT_DATA: the range, whatever follows
    assert fn(h, 0, 5, *ok, p, None) == BAD                      # 10 slots in a table of 9
    assert fn(h, 2, 4, *ok, p, None) == BAD                      # [2, 10)
    assert fn(h, 10, 0, *ok, p, None) == BAD                     # first past the table
    assert fn(h, 1, 0x80000000, *ok, p, None) == BAD             # 2 * count overflows 32 bits
    assert fn(h, 0xFFFFFFFF, 1, *ok, p, None) == BAD
    assert fn(None, 0, 1, *ok, p, None) == BAD
    assert fn(h, 0, 1, *ok, None, None) == BAD                   # conns NULL with count != 0
    assert fn(h, 0, 5, 0, R.MAC_SHA256, 0, T.PRF_SHA256, p, None) == BAD      # a bad range with an unknown cipher
    assert fn(h, 0, 1, 0, 0, 2, T.PRF_NONE, None, None) == BAD   # conns NULL with everything else unknown
    # FEATURE_UNAVAILABLE: cipher or mac, then prf, each before etm
    for cipher in (0, M.CIPHER_AES_128_GCM, M.CIPHER_CAMELLIA_256_CCM, A256 + 1, -1):
        assert fn(h, 0, 1, cipher, R.MAC_SHA256, 0, T.PRF_SHA256, p, None) == UNA, cipher
    for mac in (0, 4, -1):
        assert fn(h, 0, 1, A128, mac, 0, T.PRF_SHA256, p, None) == UNA, mac
    assert fn(h, 0, 1, A128, 4, 0, 3, p, None) == UNA            # an unknown mac with an unknown prf
    assert fn(h, 0, 1, 0, R.MAC_SHA1, 2, T.PRF_SHA256, p, None) == UNA       # an unknown cipher with a bad etm
    for prf in (T.PRF_NONE, 3, -1):
        assert fn(h, 0, 1, A128, R.MAC_SHA1, 0, prf, p, None) == UNA, prf
    assert fn(h, 0, 1, A128, R.MAC_SHA1, 2, T.PRF_NONE, p, None) == UNA      # an unknown prf with a bad etm
    # BAD_INPUT_DATA: etm, last -- also for an empty range
    for etm in (2, -1, 256):
        assert fn(h, 0, 1, A128, R.MAC_SHA1, etm, T.PRF_SHA256, p, None) == BAD, etm
        assert fn(h, 0, 0, A128, R.MAC_SHA1, etm, T.PRF_SHA256, p, None) == BAD, etm
    # count == 0 with valid arguments: 0, nothing launched, nothing loaded
    assert fn(h, 9, 0, *ok, p, None) == 0                        # an empty range at the end
    assert fn(h, 1, 0, *ok, None, None) == 0                     # conns may be NULL
    # the AEAD call still answers the CBC ids as unknown ciphers
    for cipher in (A128, A256):
        assert M.load().tlsrec_tls12_keytab_derive(h, 0, 1, cipher, T.PRF_SHA256, p, None) == UNA
    with pytest.raises(T.KeyScheduleError) as e:
        T.tls12_keytab_derive_cbc(kt, 1, 5, *ok, conns)
    assert e.value.code == BAD
    # the largest range that fits: slots 1..8; none of the refused calls loaded slot 0 or 1
    run = CL.Run([None] * 9, [CL.plain_rec(s, 50, 60 + s) for s in (0, 1)])
    out, res = run.gpu(False, kt=kt)
    assert not run.compare(False, out, res), "a refused or empty call loaded a slot"
    assert [int(x) for x in res["status"]] == [BAD, BAD]
    _derive(kt, 1, 4, A128, R.MAC_SHA256, 0, "sha256", conns, raw)
    _check_records(kt, [None] + _expected_keys("sha256", A128, R.MAC_SHA256, 0, raw, 4), [100] * 8, seed=3,
                   unloaded=[0])
    kt.close()
