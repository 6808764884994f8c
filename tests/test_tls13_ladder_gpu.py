"""GPU parity of the TLS 1.3 ladder (tls13_ladder.hip, through the C ABI): the
single-shot helpers, Finished MAC and PSK binder against the reference's own
vectors (tests/golden/tls13_handshake.json) and the hashlib ladder of
tests/tls13_ref.py, and the batch stages -- every output array bit-exact at the
workgroup edges for every (hash, psk_len, shared_len) shape, and the key-table
slots they load checked end to end by TLS 1.3 record protection."""
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
from mbedtls_amd import _abi  # noqa: E402
from mbedtls_amd import keysched as K  # noqa: E402
from tests import batchlib as B  # noqa: E402
from tests import tls13_ref as R  # noqa: E402
from tests.prng import prng_bytes  # noqa: E402

G = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "tls13_handshake.json")))
X = bytes.fromhex
DEV = torch.device("cuda")
ALG = {"sha256": K.ALG_SHA_256, "sha384": K.ALG_SHA_384}
HASHES = sorted(ALG)
# the suite fixes the hash: AES-256-GCM is the SHA-384 one
CIPHER = {"sha256": M.CIPHER_AES_128_GCM, "sha384": M.CIPHER_AES_256_GCM}
COUNTS = [1, 63, 64, 65, 130]           # one lane per connection, 64 per workgroup
PSK_LENS = [0, 1, 32, 47, 48]
SHARED_LENS = [0, 32, 48, 56, 66]
BAD, UNA = M.ERR_SSL_BAD_INPUT_DATA, M.ERR_SSL_FEATURE_UNAVAILABLE
GUARD = 32


# ---- single-shot ---------------------------------------------------------------
def test_helper_vectors():
    v = G["early_secrets"][0]
    assert tuple(x.hex() for x in K.derive_early_secrets(ALG[v["hash"]], X(v["secret"]), X(v["transcript"]))) == \
        (v["client_early_traffic_secret"], v["early_exporter_master_secret"])
    v = G["handshake_secrets"][0]
    assert tuple(x.hex() for x in K.derive_handshake_secrets(ALG[v["hash"]], X(v["secret"]), X(v["transcript"]))) == \
        (v["client_handshake_traffic_secret"], v["server_handshake_traffic_secret"])
    v = G["application_secrets"][0]
    assert tuple(x.hex() for x in K.derive_application_secrets(ALG[v["hash"]], X(v["secret"]), X(v["transcript"]))) == \
        (v["client_application_traffic_secret_N"], v["server_application_traffic_secret_N"],
         v["exporter_master_secret"])
    v = G["resumption_secrets"][0]
    assert K.derive_resumption_master_secret(ALG[v["hash"]], X(v["secret"]), X(v["transcript"])).hex() == \
        v["resumption_master_secret"]


def test_psk_binder_vector():
    v = G["psk_binder"][0]
    assert K.create_psk_binder(ALG[v["hash"]], X(v["psk"]), K.PSK_RESUMPTION, X(v["transcript"])).hex() == v["binder"]
    assert K.create_psk_binder(ALG[v["hash"]], X(v["psk"]), K.PSK_EXTERNAL, X(v["transcript"])) == \
        R.psk_binder(v["hash"], X(v["psk"]), False, X(v["transcript"]))


@pytest.mark.parametrize("hname", HASHES)
def test_single_shot_against_the_checker(hname):
    H, a = R.HLEN[hname], ALG[hname]
    s, t = prng_bytes(0x1310, H), prng_bytes(0x1311, H)
    assert K.derive_early_secrets(a, s, t) == (R.derive_secret(hname, s, b"c e traffic", t),
                                               R.derive_secret(hname, s, b"e exp master", t))
    assert K.derive_handshake_secrets(a, s, t) == (R.derive_secret(hname, s, b"c hs traffic", t),
                                                   R.derive_secret(hname, s, b"s hs traffic", t))
    ap = R.application_stage(hname, s, t, 16)
    assert K.derive_application_secrets(a, s, t) == (ap["c_ap"], ap["s_ap"], ap["exporter"])
    assert K.derive_resumption_master_secret(a, s, t) == R.derive_secret(hname, s, b"res master", t)
    assert K.calc_finished(a, s, t) == R.calc_finished(hname, s, t)
    for n in (1, 32, 48, 100):
        psk = prng_bytes(0x1320 + n, n)
        for typ in (K.PSK_EXTERNAL, K.PSK_RESUMPTION):
            assert K.create_psk_binder(a, psk, typ, t) == R.psk_binder(hname, psk, typ == K.PSK_RESUMPTION, t), (n, typ)
    # the structure: only the first Hash.length bytes of a field are written, binder_key is left alone
    out = _abi.CTls13EarlySecrets()
    ctypes.memset(ctypes.addressof(out), 0xEE, ctypes.sizeof(out))
    assert M.load().tlsrec_tls13_derive_early_secrets(a, s, t, H, ctypes.byref(out)) == 0
    assert bytes(out.binder_key) == b"\xee" * 64
    assert bytes(out.client_early_traffic_secret) == R.derive_secret(hname, s, b"c e traffic", t) + b"\xee" * (64 - H)


# ---- batch helpers -------------------------------------------------------------
def _dev(raw, shift=0):
    """bytes on the device, `shift` bytes past a 16-byte boundary"""
    buf = torch.zeros(len(raw) + 32, dtype=torch.uint8, device=DEV)
    view = buf[shift:shift + len(raw)]
    view.copy_(torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()))
    assert view.data_ptr() % 16 == shift % 16
    return view


class Out:
    """a device array of n 48-byte elements with guard bytes on both sides"""

    def __init__(self, n, shift=0):
        self.n = n
        self.buf = torch.full((GUARD + shift + 48 * n + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        self.view = self.buf[GUARD + shift:GUARD + shift + 48 * n]
        self.lo = GUARD + shift

    def read(self, H):
        """the n values; checks the guards and the zero tails"""
        raw = self.buf.cpu().numpy().tobytes()
        assert raw[:self.lo] == b"\xa5" * self.lo and raw[self.lo + 48 * self.n:] == b"\xa5" * GUARD
        el = [raw[self.lo + 48 * i:self.lo + 48 * i + 48] for i in range(self.n)]
        assert all(e[H:] == bytes(48 - H) for e in el)
        return [e[:H] for e in el]


def _conn(raw, i):
    c = raw[176 * i:176 * i + 176]
    return c[:48], c[48:128], c[128:176]


def _hs_expected(hname, cipher, raw, count, psk_len, shared_len):
    H = R.HLEN[hname]
    out = []
    for i in range(count):
        psk, shared, tr = _conn(raw, i)
        out.append(R.handshake_stage(hname, psk[:psk_len] or None, shared[:shared_len] or None, tr[:H],
                                     M.KEYLEN[cipher]))
    return out


def _slots(cipher, stages):
    """B.Batch slot tuples, client_write then server_write per connection"""
    s = []
    for st in stages:
        for side in ("c_keys", "s_keys"):
            key, iv = st[side]
            s.append((cipher, M.VERSION_TLS1_3, key, iv + bytes(4), 0))
    return s


def _encrypt(kt, slots, first, seed):
    """TLS 1.3 records, one or two per slot, protected under `kt` (None: a table
    tlsrec_keytab_load fills with `slots`, preceded by `first` others)"""
    lengths = [(53 * k) % 400 for k in range(len(slots) + 7)]
    recs = B.plaintext_records(slots, lengths, seed=seed)
    for r in recs:
        r.slot += first
    b = B.Batch([(slots[0][0], M.VERSION_TLS1_3, bytes(32), bytes(16), 0)] * first + slots, recs)
    out, res = b.run_gpu(False, kt=kt)
    return b, recs, out, res


def _records_match(kt, slots, first, seed, unloaded=()):
    """records under the derived table are byte-identical to records under a
    loaded table of the checker's keys; `unloaded` slots were never loaded"""
    b, recs, out, res = _encrypt(kt, slots, first, seed)
    _, _, want_out, want_res = _encrypt(None, slots, first, seed)
    assert [int(r["status"]) for r in want_res] == [0] * len(recs)
    assert res.tobytes() == want_res.tobytes()
    assert out.tobytes() == want_out.tobytes()
    if unloaded:
        extra = B.plaintext_records([None], [40] * len(unloaded), seed=seed + 1)
        for r, s in zip(extra, unloaded):
            r.slot = s
        _, eres = B.Batch([], extra).run_gpu(False, kt=kt)
        assert [int(r["status"]) for r in eres] == [BAD] * len(unloaded)
    return b, recs, out, res


def _cross_decrypt(enc_kt, dec_kt, slots, first, seed):
    """what one endpoint's table writes, the other's reads: even slots carry
    client -> server records, odd ones server -> client"""
    b, recs, out, res = _encrypt(enc_kt, slots, first, seed)
    sealed = []
    for i, r in enumerate(recs):
        assert int(res[i]["status"]) == 0
        o = b.offs[i]
        sealed.append(B.Rec(slot=r.slot, buf=bytearray(out[o:o + len(r.buf)].tobytes()),
                            data_offset=int(res[i]["data_offset"]), data_len=int(res[i]["data_len"]), ctr=r.ctr,
                            type=int(res[i]["type"])))
    d = B.Batch([], sealed)
    dout, dres = d.run_gpu(True, kt=dec_kt)
    for i, r in enumerate(recs):
        g = dres[i]
        assert (int(g["status"]), int(g["data_len"]), int(g["type"])) == (0, r.data_len, r.type), i
        s0 = d.offs[i] + int(g["data_offset"])
        assert dout[s0:s0 + r.data_len].tobytes() == bytes(r.buf[r.data_offset:r.data_offset + r.data_len]), i


@pytest.fixture(scope="module")
def table():
    kt = M.KeyTable(1 + 2 * max(COUNTS))
    yield kt
    kt.close()


# ---- handshake stage -----------------------------------------------------------
@pytest.mark.parametrize("shared_len", SHARED_LENS)
@pytest.mark.parametrize("psk_len", PSK_LENS)
@pytest.mark.parametrize("hname", HASHES)
def test_handshake_stage_outputs(table, hname, psk_len, shared_len):
    """every output array against the checker at the workgroup edges; first is
    odd; the run of 65 reads conns 8 bytes off a 16-byte boundary (byte loads)"""
    H, cipher = R.HLEN[hname], CIPHER[hname]
    for count in COUNTS:
        raw = prng_bytes(0x1300 + 7 * count + psk_len + 64 * shared_len, count * 176)
        conns = _dev(raw, 8 if count == 65 else 0)
        hs, fin, ms = Out(2 * count), Out(2 * count), Out(count)
        K.keytab_derive_handshake(table, 1, count, cipher, psk_len, shared_len, conns, hs.view, fin.view, ms.view)
        torch.cuda.synchronize()
        assert conns.cpu().numpy().tobytes() == raw
        want = _hs_expected(hname, cipher, raw, count, psk_len, shared_len)
        assert hs.read(H) == [w[k] for w in want for k in ("c_hs", "s_hs")], count
        assert fin.read(H) == [w[k] for w in want for k in ("c_fin", "s_fin")], count
        assert ms.read(H) == [w["master"] for w in want], count


@pytest.mark.parametrize("cipher,hname,psk_len,shared_len", [
    (M.CIPHER_AES_128_GCM, "sha256", 32, 32), (M.CIPHER_AES_256_GCM, "sha384", 0, 48),
    (M.CIPHER_CHACHA20_POLY1305, "sha256", 0, 66), (M.CIPHER_AES_128_CCM_8, "sha256", 47, 0)])
def test_handshake_slots_end_to_end(cipher, hname, psk_len, shared_len):
    """the loaded slots: records as under a loaded table of the checker's keys,
    the slots around the range untouched, and a client's and a server's table
    reading each other's records"""
    count, first = 65, 3
    raw = prng_bytes(0x13E0 + cipher, count * 176)
    conns = _dev(raw)
    tabs = []
    for _ in range(2):
        kt = M.KeyTable(first + 2 * count + 2)
        hs, ms = Out(2 * count), Out(count)
        K.keytab_derive_handshake(kt, first, count, cipher, psk_len, shared_len, conns, hs.view, None, ms.view)
        tabs.append(kt)
    torch.cuda.synchronize()
    slots = _slots(cipher, _hs_expected(hname, cipher, raw, count, psk_len, shared_len))
    _records_match(tabs[0], slots, first, seed=31, unloaded=[0, 1, 2, first + 2 * count, first + 2 * count + 1])
    client, server = tabs
    _cross_decrypt(client, server, slots, first, seed=32)
    _cross_decrypt(server, client, slots, first, seed=33)
    for kt in tabs:
        kt.close()


def test_handshake_without_finished_keys(table):
    for hname in HASHES:
        H, count = R.HLEN[hname], 65
        conns = _dev(prng_bytes(0x13F0, count * 176))
        got = []
        for with_fin in (True, False):
            hs, fin, ms = Out(2 * count), Out(2 * count), Out(count)
            K.keytab_derive_handshake(table, 1, count, CIPHER[hname], 32, 32, conns, hs.view,
                                      fin.view if with_fin else None, ms.view)
            torch.cuda.synchronize()
            got.append((hs.read(H), ms.read(H)))
            if not with_fin:
                assert fin.buf.cpu().numpy().tobytes() == b"\xa5" * fin.buf.numel()
        assert got[0] == got[1]


# ---- application stage, KeyUpdate -----------------------------------------------
@pytest.mark.parametrize("hname", HASHES)
def test_application_stage_outputs(table, hname):
    H, cipher = R.HLEN[hname], CIPHER[hname]
    for count in COUNTS:
        shift = 8 if count == 65 else 0
        mraw, traw = prng_bytes(0x1400 + count, count * 48), prng_bytes(0x1440 + count, count * 48)
        master, trs = _dev(mraw, shift), _dev(traw, shift)
        got = []
        for with_exp in (True, False):
            ap, ex = Out(2 * count, shift), Out(count, shift)
            K.keytab_derive_application(table, 1, count, cipher, master, trs, ap.view, ex.view if with_exp else None)
            torch.cuda.synchronize()
            got.append(ap.read(H))
            if not with_exp:
                assert ex.buf.cpu().numpy().tobytes() == b"\xa5" * ex.buf.numel()
        assert master.cpu().numpy().tobytes() == mraw and trs.cpu().numpy().tobytes() == traw
        want = [R.application_stage(hname, mraw[48 * i:48 * i + H], traw[48 * i:48 * i + H], M.KEYLEN[cipher])
                for i in range(count)]
        assert got[0] == got[1] == [w[k] for w in want for k in ("c_ap", "s_ap")], count
        ap, ex = Out(2 * count), Out(count)
        K.keytab_derive_application(table, 1, count, cipher, master, trs, ap.view, ex.view)
        torch.cuda.synchronize()
        assert ex.read(H) == [w["exporter"] for w in want], count


@pytest.mark.parametrize("cipher,hname", [(M.CIPHER_AES_128_GCM, "sha256"), (M.CIPHER_AES_256_GCM, "sha384"),
                                          (M.CIPHER_CHACHA20_POLY1305, "sha256")])
def test_application_slots_and_key_update(cipher, hname):
    """handshake stage -> application stage over the same slot pair -> KeyUpdate
    through tlsrec_tls13_keytab_derive on app_traffic as it stands"""
    H, count, first = R.HLEN[hname], 65, 5
    raw, traw = prng_bytes(0x1480 + cipher, count * 176), prng_bytes(0x1490 + cipher, count * 48)
    conns, trs = _dev(raw), _dev(traw)
    tabs, aps = [], []
    for _ in range(2):
        kt = M.KeyTable(first + 2 * count + 1)
        hs, ms, ap = Out(2 * count), Out(count), Out(2 * count)
        K.keytab_derive_handshake(kt, first, count, cipher, 32, 32, conns, hs.view, None, ms.view)
        K.keytab_derive_application(kt, first, count, cipher, ms.view, trs, ap.view, None)
        tabs.append(kt)
        aps.append(ap)
    torch.cuda.synchronize()
    hsx = _hs_expected(hname, cipher, raw, count, 32, 32)
    want = [R.application_stage(hname, hsx[i]["master"], traw[48 * i:48 * i + H], M.KEYLEN[cipher]) for i in range(count)]
    secrets = [w[k] for w in want for k in ("c_ap", "s_ap")]
    assert aps[0].read(H) == secrets
    slots = _slots(cipher, want)
    _records_match(tabs[0], slots, first, seed=41, unloaded=[0, first - 1, first + 2 * count])
    _cross_decrypt(tabs[0], tabs[1], slots, first, seed=42)
    _cross_decrypt(tabs[1], tabs[0], slots, first, seed=43)
    K.keytab_derive(tabs[0], first, 2 * count, cipher, aps[0].view, key_update=True)
    torch.cuda.synchronize()
    nxt = [R.next_generation(hname, s) for s in secrets]
    assert aps[0].read(H) == nxt
    keys = [R.traffic_keys(hname, s, M.KEYLEN[cipher]) for s in nxt]
    _records_match(tabs[0], [(cipher, M.VERSION_TLS1_3, k, iv + bytes(4), 0) for k, iv in keys], first, seed=44)
    for kt in tabs:
        kt.close()


# ---- Finished, Derive-Secret ----------------------------------------------------
@pytest.mark.parametrize("hname", HASHES)
def test_batch_verify_data_and_derive_secret(hname):
    H, a = R.HLEN[hname], ALG[hname]
    for count in COUNTS:
        shift = 8 if count == 65 else 0
        kraw, traw = prng_bytes(0x1500 + count, count * 48), prng_bytes(0x1540 + count, count * 48)
        keys, trs = _dev(kraw, shift), _dev(traw, shift)
        ks = [kraw[48 * i:48 * i + H] for i in range(count)]
        ts = [traw[48 * i:48 * i + H] for i in range(count)]
        out = Out(count, shift)
        K.batch_verify_data(a, keys, trs, out.view, count)
        torch.cuda.synchronize()
        assert out.read(H) == [R.verify_data(hname, k, t) for k, t in zip(ks, ts)], count
        for label in (b"res master", b"x", b"twelve chars", b""):
            out = Out(count, shift)
            K.batch_derive_secret(a, label, keys, trs, out.view, count)
            torch.cuda.synchronize()
            assert out.read(H) == [R.derive_secret(hname, k, label, t) for k, t in zip(ks, ts)], (count, label)
        assert keys.cpu().numpy().tobytes() == kraw and trs.cpu().numpy().tobytes() == traw


def test_every_label_length():
    for hname, n in itertools.product(HASHES, range(13)):
        H, label = R.HLEN[hname], bytes(0x61 + k for k in range(n))
        kraw, traw = prng_bytes(0x1580 + n, 3 * 48), prng_bytes(0x15A0 + n, 3 * 48)
        out = Out(3)
        K.batch_derive_secret(ALG[hname], label, _dev(kraw), _dev(traw), out.view, 3)
        torch.cuda.synchronize()
        assert out.read(H) == [R.derive_secret(hname, kraw[48 * i:48 * i + H], label, traw[48 * i:48 * i + H])
                               for i in range(3)], (hname, n)


# ---- one connection: the batch is the single-shot ladder -------------------------
@pytest.mark.parametrize("hname", HASHES)
def test_one_connection_equals_the_single_shot_ladder(table, hname):
    H, a, cipher = R.HLEN[hname], ALG[hname], CIPHER[hname]
    raw, tr2, tr3 = prng_bytes(0x1600, 176), prng_bytes(0x1601, 48), prng_bytes(0x1602, 48)
    psk, shared, tr = _conn(raw, 0)
    hs, fin, ms, ap, ex, vd, rm = Out(2), Out(2), Out(1), Out(2), Out(1), Out(2), Out(1)
    K.keytab_derive_handshake(table, 1, 1, cipher, 32, 32, _dev(raw), hs.view, fin.view, ms.view)
    K.batch_verify_data(a, fin.view, _dev(tr2 + tr2), vd.view, 2)
    K.keytab_derive_application(table, 1, 1, cipher, ms.view, _dev(tr2), ap.view, ex.view)
    K.batch_derive_secret(a, b"res master", ms.view, _dev(tr3), rm.view, 1)
    torch.cuda.synchronize()
    early = K.evolve_secret(a, None, psk[:32])
    hsec = K.evolve_secret(a, early, shared[:32])
    c, s = K.derive_handshake_secrets(a, hsec, tr[:H])
    master = K.evolve_secret(a, hsec, None)
    assert hs.read(H) == [c, s] and ms.read(H) == [master]
    assert fin.read(H) == [K.hkdf_expand_label(a, x, b"finished", b"", H) for x in (c, s)]
    assert vd.read(H) == [K.calc_finished(a, x, tr2[:H]) for x in (c, s)]
    ca, sa, exp = K.derive_application_secrets(a, master, tr2[:H])
    assert ap.read(H) == [ca, sa] and ex.read(H) == [exp]
    assert rm.read(H) == [K.derive_resumption_master_secret(a, master, tr3[:H])]
    ck, civ, sk, siv = K.make_traffic_keys(a, ca, sa, M.KEYLEN[cipher], 12)
    _records_match(table, [(cipher, M.VERSION_TLS1_3, ck, civ + bytes(4), 0),
                           (cipher, M.VERSION_TLS1_3, sk, siv + bytes(4), 0)], 1, seed=51)


# ---- arguments -------------------------------------------------------------------
def test_batch_argument_errors_in_order():
    L = M.load()
    kt = M.KeyTable(9)
    c = M.CIPHER_AES_128_GCM
    conns = _dev(prng_bytes(1, 4 * 176))
    o = Out(8)
    p, q = conns.data_ptr(), o.view.data_ptr()
    hs, app = L.tlsrec_tls13_keytab_derive_handshake, L.tlsrec_tls13_keytab_derive_application
    # BAD_INPUT_DATA wins over a cipher and a shared_len that would be FEATURE_UNAVAILABLE
    for cipher, sl in ((c, 32), (0, 33)):
        assert hs(None, 0, 1, cipher, 0, sl, p, q, q, q, None) == BAD
        assert hs(kt.handle, 0, 1, cipher, 0, sl, None, q, q, q, None) == BAD
        assert hs(kt.handle, 0, 1, cipher, 0, sl, p, None, q, q, None) == BAD
        assert hs(kt.handle, 0, 1, cipher, 0, sl, p, q, q, None, None) == BAD
        assert hs(kt.handle, 0, 1, cipher, 49, sl, p, q, q, q, None) == BAD
        assert hs(kt.handle, 0, 5, cipher, 0, sl, p, q, q, q, None) == BAD          # 10 slots in a table of 9
        assert hs(kt.handle, 10, 0, cipher, 0, sl, p, q, q, q, None) == BAD
        assert hs(kt.handle, 1, 0x80000000, cipher, 0, sl, p, q, q, q, None) == BAD
        assert app(None, 0, 1, cipher, q, q, q, q, None) == BAD
        assert app(kt.handle, 0, 1, cipher, None, q, q, q, None) == BAD
        assert app(kt.handle, 0, 1, cipher, q, None, q, q, None) == BAD
        assert app(kt.handle, 0, 1, cipher, q, q, None, q, None) == BAD
        assert app(kt.handle, 2, 4, cipher, q, q, q, q, None) == BAD
    for cipher in (0, M.CIPHER_CAMELLIA_256_CCM + 1):
        assert hs(kt.handle, 0, 1, cipher, 0, 32, p, q, q, q, None) == UNA
        assert app(kt.handle, 0, 1, cipher, q, q, q, q, None) == UNA
    for sl in (1, 31, 33, 64, 80, 256):
        assert hs(kt.handle, 0, 1, c, 0, sl, p, q, q, q, None) == UNA
    assert hs(kt.handle, 9, 0, c, 48, 66, None, None, None, None, None) == 0
    assert app(kt.handle, 9, 0, c, None, None, None, None, None) == 0
    torch.cuda.synchronize()
    # no refused call wrote anything or loaded a slot
    assert o.buf.cpu().numpy().tobytes() == b"\xa5" * o.buf.numel()
    extra = B.plaintext_records([None], [40] * 9, seed=2)
    for s, r in enumerate(extra):
        r.slot = s
    _, eres = B.Batch([], extra).run_gpu(False, kt=kt)
    assert [int(r["status"]) for r in eres] == [BAD] * 9
    kt.close()
