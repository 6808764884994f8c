"""GPU parity of the TLS 1.2 / DTLS 1.2 key derivation (tls12_batch.hip, through
the C ABI): the reference's own PRF vectors (tests/golden/tls12_prf.json), the
single-shot calls against two independent checkers (P_hash over hashlib and
OpenSSL's EVP_KDF "TLS1-PRF", tests/tls12_ref.py) on the sizes where the block,
padding and key-hashing branches change, and the batch expansion into a key
table checked end to end by TLS 1.2 record encryption and a DTLS 1.2 exchange
between a server's and a client's table.  Everything is bit-exact."""
import ctypes
import itertools
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

import mbedtls_amd as M  # noqa: E402
from mbedtls_amd import dtls as D  # noqa: E402
from mbedtls_amd import stream as S  # noqa: E402
from mbedtls_amd import tls12 as T  # noqa: E402
from tests import batchlib as B  # noqa: E402
from tests.prng import prng_bytes  # noqa: E402
from tests.tls12_ref import evp_tls1_prf, p_hash, split_key_block  # noqa: E402

G = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "tls12_prf.json")))
X = bytes.fromhex
PRF = {"sha256": T.PRF_SHA256, "sha384": T.PRF_SHA384}
PRFS = sorted(PRF)
CIPHERS = sorted(M.KEYLEN)
DEV = torch.device("cuda")


def _ivlen(cipher):
    return 12 if cipher == M.CIPHER_CHACHA20_POLY1305 else 4


def _label(seed, n):
    """n label bytes without a NUL (the label is a C string)"""
    return bytes(1 + b % 255 for b in prng_bytes(seed, n))


def _both(hname, secret, seed, n):
    """the expected PRF output: P_hash over hashlib, cross-checked by OpenSSL
    where its provider takes the inputs (non-empty secret and seed)"""
    want = p_hash(hname, secret, seed, n)
    if secret and seed and n:
        assert evp_tls1_prf(hname, secret, seed, n) == want
    return want


@pytest.mark.parametrize("v", G["vectors"], ids=lambda v: v["where"])
def test_reference_vectors(v):
    want = X(v["expected"])
    got = T.tls_prf(PRF[v["prf"]], X(v["secret"]), v["label"].encode(), X(v["random"]), len(want))
    assert got.hex() == v["expected"]


DLEN = [1, 31, 32, 33, 47, 48, 49, 95, 96, 97, 256, 1000]
SLEN = [0, 1, 48, 64, 65, 128, 129, 200]
SEEDLEN = [0, 1, 22, 23, 24, 55, 56, 64, 78, 79, 80, 111, 112, 128]


@pytest.mark.parametrize("hname", PRFS)
def test_tls_prf_edge_sizes(hname):
    """Every output length with every secret length and with every seed
    length, every (secret length, seed length) pair, and every output length
    at the key-expansion shape (48, 13 + 64)."""
    cases = [(48, 77, d) for d in DLEN]
    for idx, (sl, tot) in enumerate(itertools.product(SLEN, SEEDLEN)):
        cases.append((sl, tot, DLEN[idx % len(DLEN)]))
    cases += [(sl, 77, d) for sl, d in itertools.product(SLEN, DLEN)]
    cases += [(48, tot, d) for tot, d in itertools.product(SEEDLEN, DLEN)]
    seen_s, seen_t, seen_p = set(), set(), set()
    for k, (sl, tot, dl) in enumerate(cases):
        ll = min(tot, (5, 13, 22, 0)[k % 4])
        secret, label, rnd = prng_bytes(0x100 + k, sl), _label(0x200 + k, ll), prng_bytes(0x300 + k, tot - ll)
        want = _both(hname, secret, label + rnd, dl)
        assert T.tls_prf(PRF[hname], secret, label, rnd, dl) == want, (sl, tot, dl)
        seen_s.add((sl, dl))
        seen_t.add((tot, dl))
        seen_p.add((sl, tot))
    assert seen_s >= set(itertools.product(SLEN, DLEN)) and seen_t >= set(itertools.product(SEEDLEN, DLEN))
    assert seen_p >= set(itertools.product(SLEN, SEEDLEN))


@pytest.mark.parametrize("hname", PRFS)
def test_tls_prf_zero_length_output(hname):
    L = M.load()
    out = ctypes.create_string_buffer(b"\xaa" * 64, 64)
    assert L.tlsrec_tls_prf(PRF[hname], bytes(48), 48, b"label", bytes(64), 64, out, 0) == 0
    assert out.raw == b"\xaa" * 64
    assert T.tls_prf(PRF[hname], bytes(48), b"label", bytes(64), 0) == b""


def test_tls_prf_arena_limit():
    """the one documented divergence: inputs + output beyond the 32 KiB arena"""
    for args in ((bytes(48), b"l", bytes(64), 32768), (bytes(20000), b"l", bytes(64), 16000),
                 (bytes(48), b"l", bytes(40000), 16)):
        with pytest.raises(T.KeyScheduleError) as e:
            T.tls_prf(T.PRF_SHA256, *args)
        assert e.value.code == M.ERR_SSL_BAD_INPUT_DATA
    n = 32768 - 48 - 16 - 64
    assert T.tls_prf(T.PRF_SHA256, bytes(48), b"l", bytes(64), n) == p_hash("sha256", bytes(48), b"l" + bytes(64), n)


@pytest.mark.parametrize("hname", PRFS)
def test_compute_master(hname):
    for k, pl in enumerate((32, 48, 66)):
        pms = prng_bytes(0x400 + k, pl)
        rnd = prng_bytes(0x410 + k, 64)
        assert T.tls12_compute_master(PRF[hname], pms, rnd) == _both(hname, pms, b"master secret" + rnd, 48)
        for hl in (32, 48):         # session hash of a SHA-256 / SHA-384 suite
            sh = prng_bytes(0x420 + 8 * k + hl, hl)
            assert T.tls12_compute_master(PRF[hname], pms, sh, extended_ms=True) == \
                _both(hname, pms, b"extended master secret" + sh, 48)


@pytest.mark.parametrize("hname", PRFS)
def test_make_keys_every_cipher(hname):
    for c in CIPHERS:
        master, rb = prng_bytes(0x500 + c, 48), prng_bytes(0x540 + c, 64)
        kl, il = M.KEYLEN[c], _ivlen(c)
        blk = _both(hname, master, b"key expansion" + rb, 2 * kl + 2 * il)
        assert T.tls12_make_keys(PRF[hname], c, master, rb) == split_key_block(blk, kl, il), c
    with pytest.raises(T.KeyScheduleError) as e:
        T.tls12_make_keys(PRF[hname], 0, bytes(48), bytes(64))
    assert e.value.code == M.ERR_SSL_FEATURE_UNAVAILABLE


@pytest.mark.parametrize("hname", PRFS)
def test_export_keying_material(hname):
    master = prng_bytes(0x600, 48)
    srv, cli = prng_bytes(0x601, 32), prng_bytes(0x602, 32)
    assert srv != cli
    rb = srv + cli                       # handshake->randbytes after the swap
    label = b"EXPORTER-test label"
    for n in (1, 32, 100):
        assert T.tls12_export_keying_material(PRF[hname], master, rb, label, None, n) == \
            _both(hname, master, label + cli + srv, n)
        for cl in (0, 1, 300):
            ctx = prng_bytes(0x610 + cl, cl)
            assert T.tls12_export_keying_material(PRF[hname], master, rb, label, ctx, n) == \
                _both(hname, master, label + cli + srv + cl.to_bytes(2, "big") + ctx, n), (n, cl)
    with pytest.raises(T.KeyScheduleError) as e:
        T.tls12_export_keying_material(PRF[hname], master, rb, label, bytes(65536), 32)
    assert e.value.code == M.ERR_SSL_BAD_INPUT_DATA
    # a context the reference would take but the arena does not hold
    with pytest.raises(T.KeyScheduleError) as e:
        T.tls12_export_keying_material(PRF[hname], master, rb, label, bytes(40000), 32)
    assert e.value.code == M.ERR_SSL_BAD_INPUT_DATA


# ---- batch ---------------------------------------------------------------------
def _conns(seed, count):
    raw = prng_bytes(seed, count * 112)
    return raw, torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(DEV)


def _expected_slots(hname, cipher, raw, count):
    """B.Batch slot tuples of the 2 * count slots: client_write, server_write per connection"""
    kl, il = M.KEYLEN[cipher], _ivlen(cipher)
    slots = []
    for i in range(count):
        master, rb = raw[112 * i:112 * i + 48], raw[112 * i + 48:112 * i + 112]
        ck, civ, sk, siv = split_key_block(p_hash(hname, master, b"key expansion" + rb, 2 * kl + 2 * il), kl, il)
        slots.append((cipher, M.VERSION_TLS1_2, ck, civ + bytes(16 - il), 0))
        slots.append((cipher, M.VERSION_TLS1_2, sk, siv + bytes(16 - il), 0))
    return slots


def _check_records(kt, slots, first, lengths, seed, unloaded=()):
    """Encrypt TLS 1.2 records (slot k of `slots` gets records k, k + len(slots), ...)
    under the derived table, against the oracle record layer; in the same batch
    every slot id of `unloaded` gets a record, which must come back
    BAD_INPUT_DATA with its buffer untouched (a slot never loaded)."""
    recs = B.plaintext_records(slots, lengths, seed=seed)
    for r in recs:
        r.slot += first
    ngood = len(recs)
    extra = B.plaintext_records([None], [40 + 3 * k for k in range(len(unloaded))], seed=seed + 1)
    for r, s in zip(extra, unloaded):
        r.slot = s
    # the unloaded records interleaved at the front, the middle and the end
    order = list(range(ngood))
    for k in range(len(extra)):
        order.insert(k * len(order) // max(1, len(extra) - 1), ngood + k)
    allrecs = recs + extra
    b = B.Batch([], [allrecs[i] for i in order])
    out, res = b.run_gpu(False, kt=kt)
    good = B.Batch([(slots[0][0], M.VERSION_TLS1_2, bytes(16), bytes(16), 0)] * first + slots, recs)
    o_recs, o_stats = good.run_oracle(False)
    for pos, i in enumerate(order):
        r, g, o = allrecs[i], res[pos], b.offs[pos]
        buf = bytes(out[o:o + len(r.buf)])
        if i >= ngood:
            assert int(g["status"]) == M.ERR_SSL_BAD_INPUT_DATA and buf == bytes(r.buf), (r.slot, int(g["status"]))
            continue
        want = o_recs[i]
        assert (int(g["status"]), int(g["data_offset"]), int(g["data_len"]), int(g["type"])) == \
            (o_stats[i], want.data_offset, want.data_len, want.type), (i, r.slot)
        assert o_stats[i] == 0 and buf == bytes(want.buf), (i, r.slot)


@pytest.mark.parametrize("cipher", CIPHERS)
@pytest.mark.parametrize("hname", PRFS)
def test_keytab_derive_end_to_end(cipher, hname):
    """Device connections -> key expansion -> split -> key table -> TLS 1.2
    record encryption under both directions' slots, against P_hash + the
    oracle's record layer; the slots around the range stay unloaded."""
    count, first = 130, 3
    raw, conns = _conns(0xC0 + 2 * cipher + (hname == "sha384"), count)
    kt = M.KeyTable(first + 2 * count + 2)
    T.tls12_keytab_derive(kt, first, count, cipher, PRF[hname], conns)
    torch.cuda.synchronize()
    assert conns.cpu().numpy().tobytes() == raw
    slots = _expected_slots(hname, cipher, raw, count)
    lengths = [int(x) % 1500 for x in np.frombuffer(prng_bytes(9 + cipher, 4 * count), dtype=np.uint16)]
    _check_records(kt, slots, first, lengths, seed=91,
                   unloaded=[0, 1, 2, first + 2 * count, first + 2 * count + 1])
    kt.close()


@pytest.mark.parametrize("hname", PRFS)
@pytest.mark.parametrize("count,unaligned", [(1, False), (63, False), (64, False), (65, False), (65, True)])
def test_keytab_derive_workgroup_edges(hname, count, unaligned):
    """one lane per connection, 64 per workgroup; an array that is not
    16-byte aligned takes the byte-load path"""
    cipher = M.CIPHER_AES_256_GCM
    raw = prng_bytes(0xE0 + count, count * 112)
    buf = torch.zeros(count * 112 + 16, dtype=torch.uint8, device=DEV)
    off = 1 if unaligned else 0
    conns = buf[off:off + count * 112]
    conns.copy_(torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()))
    assert (conns.data_ptr() % 16 != 0) == unaligned
    kt = M.KeyTable(2 * count)
    T.tls12_keytab_derive(kt, 0, count, cipher, PRF[hname], conns)
    torch.cuda.synchronize()
    assert conns.cpu().numpy().tobytes() == raw
    slots = _expected_slots(hname, cipher, raw, count)
    _check_records(kt, slots, 0, [(37 * k) % 300 for k in range(2 * count)], seed=17)
    kt.close()


def _dtls_send(kt, jobs):
    """jobs: (slot, plaintext, out_ctr) -> one datagram each"""
    d = np.zeros(len(jobs), dtype=S.STREAM_OUT)
    pos_in = pos_out = 0
    where = []
    for i, (slot, pt, c8) in enumerate(jobs):
        d[i]["in_off"], d[i]["in_len"], d[i]["slot"], d[i]["out_off"], d[i]["type"] = pos_in, len(pt), slot, pos_out, 23
        d[i]["out_ctr"] = np.frombuffer(c8, dtype=np.uint8)
        where.append((pos_in, pos_out))
        pos_in += (len(pt) + 128) // 128 * 128
        pos_out += (len(pt) + 64 + 128) // 128 * 128
    ina = np.zeros(pos_in, dtype=np.uint8)
    for (slot, pt, c8), (pi, _) in zip(jobs, where):
        ina[pi:pi + len(pt)] = np.frombuffer(pt, dtype=np.uint8)
    tin = torch.from_numpy(ina).to(DEV)
    tout = torch.zeros(pos_out, dtype=torch.uint8, device=DEV)
    nmax = len(jobs) + 1
    recs = torch.zeros(nmax * 40, dtype=torch.uint8, device=DEV)
    res = torch.zeros(nmax * 16, dtype=torch.uint8, device=DEV)
    sres = torch.zeros(len(jobs) * 32, dtype=torch.uint8, device=DEV)
    assert D.encrypt(kt, d, len(jobs), tin, tout, recs, res, nmax, sres) == len(jobs)
    torch.cuda.synchronize()
    o = tout.cpu().numpy()
    sr = sres.cpu().numpy().view(S.STREAM_OUT_RES)
    assert [(int(r["status"]), int(r["nrec"])) for r in sr] == [(0, 1)] * len(jobs)
    return [o[po:po + int(r["out_len"])].tobytes() for (_, po), r in zip(where, sr)]


def _dtls_receive(kt, conns):
    """conns: (slot, [datagram bytes]) -> per connection the accepted plaintexts, in order"""
    d = np.zeros(len(conns), dtype=D.DTLS_IN)
    dgl, pos = [], 0
    for i, (slot, dgs) in enumerate(conns):
        d[i]["first_dgram"], d[i]["ndgram"], d[i]["slot"] = len(dgl), len(dgs), slot
        d[i]["in_epoch"], d[i]["flags"] = 1, M.DTLS_ANTI_REPLAY
        for g in dgs:
            dgl.append((pos, g))
            pos += (len(g) + 128) // 128 * 128
    a = np.zeros(pos, dtype=np.uint8)
    dg = np.zeros(len(dgl), dtype=D.DGRAM)
    for k, (p, g) in enumerate(dgl):
        a[p:p + len(g)] = np.frombuffer(g, dtype=np.uint8)
        dg[k]["off"], dg[k]["len"] = p, len(g)
    ta = torch.from_numpy(a).to(DEV)
    nmax = len(dgl) + 1
    recs = torch.zeros(nmax * 40, dtype=torch.uint8, device=DEV)
    res = torch.zeros(nmax * 16, dtype=torch.uint8, device=DEV)
    disp = torch.zeros(nmax, dtype=torch.int32, device=DEV)
    cres = torch.zeros(len(conns) * 48, dtype=torch.uint8, device=DEV)
    assert D.decrypt(kt, d, len(conns), dg, len(dgl), ta, recs, res, disp, nmax, cres) == len(dgl)
    torch.cuda.synchronize()
    a = ta.cpu().numpy()
    rc, rs = recs.cpu().numpy().view(M.BATCH_REC), res.cpu().numpy().view(M.BATCH_RES)
    dp, cr = disp.cpu().numpy(), cres.cpu().numpy().view(D.DTLS_IN_RES)
    got = []
    for i, (slot, dgs) in enumerate(conns):
        c = cr[i]
        assert (int(c["status"]), int(c["nrec"]), int(c["naccepted"])) == (0, len(dgs), len(dgs)), i
        f = int(c["first"])
        pts = []
        for k in range(len(dgs)):
            assert int(dp[f + k]) == 0 and int(rs[f + k]["status"]) == 0 and int(rs[f + k]["type"]) == 23
            s0 = int(rc[f + k]["buf_off"]) + int(rs[f + k]["data_offset"])
            pts.append(a[s0:s0 + int(rs[f + k]["data_len"])].tobytes())
        got.append(pts)
    return got


@pytest.mark.parametrize("cipher,hname", [(M.CIPHER_AES_128_GCM, "sha256"), (M.CIPHER_CHACHA20_POLY1305, "sha256"),
                                          (M.CIPHER_AES_128_GCM, "sha384")])
def test_dtls_server_and_client_tables(cipher, hname):
    """A server's and a client's table derived from the same connections:
    DTLS 1.2 datagrams written by one side are accepted by the other with the
    plaintext restored, in both directions (each side encrypts with its own
    write key and decrypts with the peer's)."""
    nconn, ngram, first = 4, 3, 1
    raw, conns = _conns(0xD715 + cipher, nconn)
    tabs = {}
    for ep in (T.IS_CLIENT, T.IS_SERVER):
        tabs[ep] = M.KeyTable(first + 2 * nconn)
        T.tls12_keytab_derive(tabs[ep], first, nconn, cipher, PRF[hname], conns)
    torch.cuda.synchronize()
    for sender, receiver in ((T.IS_CLIENT, T.IS_SERVER), (T.IS_SERVER, T.IS_CLIENT)):
        jobs, pts = [], []
        for i in range(nconn):
            enc, _ = T.tls12_slots(first, i, sender)
            pts.append([prng_bytes(0x900 + 16 * i + k + 64 * sender, (1, 200, 1400)[k]) for k in range(ngram)])
            for k in range(ngram):
                jobs.append((enc, pts[i][k], (1).to_bytes(2, "big") + (5 * i + k).to_bytes(6, "big")))
        grams = _dtls_send(tabs[sender], jobs)
        for g, (_, pt, _) in zip(grams, jobs):
            assert g[:3] == b"\x17\xfe\xfd" and (len(pt) < 16 or pt not in g)
        rx = [(T.tls12_slots(first, i, receiver)[1], grams[ngram * i:ngram * (i + 1)]) for i in range(nconn)]
        assert _dtls_receive(tabs[receiver], rx) == pts
    for kt in tabs.values():
        kt.close()


def test_keytab_derive_argument_checks():
    L = M.load()
    _, conns = _conns(1, 4)
    p = conns.data_ptr()
    kt = M.KeyTable(9)                      # odd capacity: slots 0..8
    fn = L.tlsrec_tls12_keytab_derive
    ok = (M.CIPHER_AES_128_GCM, T.PRF_SHA256, p, None)
    bad, una = M.ERR_SSL_BAD_INPUT_DATA, M.ERR_SSL_FEATURE_UNAVAILABLE
    assert fn(kt.handle, 0, 5, *ok) == bad                  # 10 slots in a table of 9
    assert fn(kt.handle, 2, 4, *ok) == bad                  # [2, 10)
    assert fn(kt.handle, 10, 0, *ok) == bad                 # first past the table
    assert fn(kt.handle, 1, 0x80000000, *ok) == bad         # 2 * count overflows 32 bits
    assert fn(kt.handle, 0xFFFFFFFF, 1, *ok) == bad
    assert fn(kt.handle, 9, 0, *ok) == 0                    # an empty range at the end
    assert fn(None, 0, 1, *ok) == bad
    assert fn(kt.handle, 0, 1, M.CIPHER_AES_128_GCM, T.PRF_SHA256, None, None) == bad
    assert fn(kt.handle, 0, 0, M.CIPHER_AES_128_GCM, T.PRF_SHA256, None, None) == 0
    assert fn(kt.handle, 0, 1, 0, T.PRF_SHA256, p, None) == una
    assert fn(kt.handle, 0, 1, M.CIPHER_CAMELLIA_256_CCM + 1, T.PRF_SHA256, p, None) == una
    assert fn(kt.handle, 0, 1, M.CIPHER_AES_128_GCM, T.PRF_NONE, p, None) == una
    assert fn(kt.handle, 0, 1, M.CIPHER_AES_128_GCM, 3, p, None) == una
    # the largest range that fits: slots 1..8
    with pytest.raises(T.KeyScheduleError) as e:
        T.tls12_keytab_derive(kt, 1, 5, M.CIPHER_AES_128_GCM, T.PRF_SHA256, conns)
    assert e.value.code == bad
    raw, conns = _conns(1, 4)
    T.tls12_keytab_derive(kt, 1, 4, M.CIPHER_AES_128_GCM, T.PRF_SHA256, conns)
    torch.cuda.synchronize()
    # slots 1..8 hold the keys; none of the refused calls loaded slot 0
    _check_records(kt, _expected_slots("sha256", M.CIPHER_AES_128_GCM, raw, 4), 1, [100] * 8, seed=3, unloaded=[0])
    kt.close()
