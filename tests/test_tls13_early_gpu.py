"""GPU parity of the resumed-handshake batches (tls13_ladder.hip, through the C ABI):
tlsrec_tls13_batch_psk_binder, tlsrec_tls13_keytab_derive_early and
tlsrec_tls13_batch_ticket_psk against the reference's RFC 8448 vectors and the
hashlib checker of tests/tls13_early_ref.py -- every output array bit-exact at
the workgroup edges, aligned and 4 bytes off, the binder compare on offered
binders that differ in their first bit, their last bit or only past Hash.length,
the loaded slots checked end to end by TLS 1.3 record protection, and the
calls composed with the ladder stages around them."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

import mbedtls_amd as M  # noqa: E402
from mbedtls_amd import keysched as K  # noqa: E402
from tests import batchlib as B  # noqa: E402
from tests import tls13_early_ref as E  # noqa: E402
from tests import tls13_ref as R  # noqa: E402
from tests.prng import prng_bytes  # noqa: E402

HERE = os.path.dirname(__file__)
KEYS = json.load(open(os.path.join(HERE, "golden", "tls13_keys.json")))
G = json.load(open(os.path.join(HERE, "golden", "tls13_handshake.json")))
X = bytes.fromhex
DEV = torch.device("cuda")
ALG = {"sha256": K.ALG_SHA_256, "sha384": K.ALG_SHA_384}
HASHES = sorted(ALG)
CIPHER = {"sha256": M.CIPHER_AES_128_GCM, "sha384": M.CIPHER_AES_256_GCM}
HNAME = {M.CIPHER_AES_128_GCM: "sha256", M.CIPHER_AES_256_GCM: "sha384", M.CIPHER_CHACHA20_POLY1305: "sha256"}
COUNTS = [1, 63, 64, 65, 130]           # one lane per connection, 64 per workgroup
PSK_LENS = [1, 32, 47, 48]
TYPES = [K.PSK_RESUMPTION, K.PSK_EXTERNAL]
SHIFTS = [0, 4]                         # every array 16-byte aligned / 4 bytes off (the byte paths)
BAD, UNA = M.ERR_SSL_BAD_INPUT_DATA, M.ERR_SSL_FEATURE_UNAVAILABLE
GUARD = 32
CONN = K.PSK_CONN_BYTES


def _dev(raw, shift=0):
    """bytes on the device, `shift` bytes past a 16-byte boundary"""
    buf = torch.zeros(len(raw) + 32, dtype=torch.uint8, device=DEV)
    view = buf[shift:shift + len(raw)]
    view.copy_(torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()))
    assert view.data_ptr() % 16 == shift % 16
    return view


class Out:
    """a device array of n elements of `el` bytes with guard bytes (0xA5) on both sides"""

    def __init__(self, n, shift=0, el=48):
        self.n, self.el = n, el
        self.buf = torch.full((GUARD + shift + el * n + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        self.view = self.buf[GUARD + shift:GUARD + shift + el * n]
        self.lo = GUARD + shift
        assert self.view.data_ptr() % 16 == shift % 16

    def raw(self):
        raw = self.buf.cpu().numpy().tobytes()
        assert raw[:self.lo] == b"\xa5" * self.lo and raw[self.lo + self.el * self.n:] == b"\xa5" * GUARD
        return raw[self.lo:self.lo + self.el * self.n]

    def read(self, H):
        """the n values of a 48-byte array; checks the guards and the zero tails"""
        raw = self.raw()
        el = [raw[48 * i:48 * i + 48] for i in range(self.n)]
        assert all(e[H:] == bytes(48 - H) for e in el)
        return [e[:H] for e in el]

    def words(self):
        """a uint32 array (match)"""
        return np.frombuffer(self.raw(), dtype="<u4").tolist()

    def untouched(self):
        return self.buf.cpu().numpy().tobytes() == b"\xa5" * self.buf.numel()


def _expected(hname, raw, count, psk_len, psk_type, key_len):
    H = R.HLEN[hname]
    out = []
    for i in range(count):
        c = raw[CONN * i:CONN * i + CONN]
        out.append(E.early_stage(hname, c[:psk_len], psk_type == K.PSK_RESUMPTION, c[48:48 + H], c[96:96 + H], key_len))
    return out


def _offered(binders, H, seed):
    """48-byte offered binders and the match vector they must give: the correct
    binder, except i % 5 == 2 (bit 0 of byte 0 flipped), i % 5 == 4 (bit 7 of
    byte H - 1 flipped) and i % 5 == 0 (only bytes past H differ: still a match)"""
    raw, want = bytearray(), []
    for i, b in enumerate(binders):
        o = bytearray(b + bytes(48 - H))
        ok = 1
        if i % 5 == 2:
            o[0] ^= 0x01
            ok = 0
        elif i % 5 == 4:
            o[H - 1] ^= 0x80
            ok = 0
        elif i % 5 == 0:
            o[H:] = bytes(x | 1 for x in prng_bytes(seed + i, 48 - H))
        raw += o
        want.append(ok)
    return bytes(raw), want


# ---- the reference's vectors ---------------------------------------------------------
def test_rfc8448_chain_through_the_batch_calls():
    """test_suite_ssl.data:2681 -> :2850 -> :2768 at count = 1"""
    t = [v for v in KEYS["expand_label"] if v["label"] == "resumption"][0]
    b, e = G["psk_binder"][0], G["early_secrets"][0]
    a, H, cipher = K.ALG_SHA_256, 32, M.CIPHER_AES_128_GCM
    nonce = X(t["ctx"])
    psk = Out(1)
    K.batch_ticket_psk(a, len(nonce), _dev(X(t["secret"]) + bytes(16)), _dev(nonce + b"\xff" * (32 - len(nonce))),
                       psk.view, 1)
    torch.cuda.synchronize()
    assert psk.read(H) == [X(t["expected"])] == [X(b["psk"])]
    conn = psk.raw() + X(b["transcript"]) + bytes(16) + X(e["transcript"]) + bytes(16)
    conns = _dev(conn)
    off, want = _offered([X(b["binder"])], H, 1)
    for typ, ok in ((K.PSK_RESUMPTION, 1), (K.PSK_EXTERNAL, 0)):
        bd, mt = Out(1), Out(1, el=4)
        K.batch_psk_binder(a, H, typ, conns, _dev(off), bd.view, mt.view, 1)
        torch.cuda.synchronize()
        assert (bd.read(H) == [X(b["binder"])]) == bool(ok) and mt.words() == [ok]
    kt = M.KeyTable(4)
    bd, mt, ce, ex = Out(1), Out(1, el=4), Out(1), Out(1)
    K.keytab_derive_early(kt, 2, 1, cipher, H, K.PSK_RESUMPTION, conns, _dev(off), bd.view, mt.view, ce.view, ex.view)
    torch.cuda.synchronize()
    assert bd.read(H) == [X(b["binder"])] and mt.words() == [1]
    assert ce.read(H) == [X(e["client_early_traffic_secret"])]
    assert ex.read(H) == [X(e["early_exporter_master_secret"])]
    _slots_decrypt(kt, cipher, [R.traffic_keys("sha256", X(e["client_early_traffic_secret"]), 16)], 2, seed=5)
    kt.close()


# ---- the binder ------------------------------------------------------------------------
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("psk_type", TYPES)
@pytest.mark.parametrize("psk_len", PSK_LENS)
@pytest.mark.parametrize("hname", HASHES)
def test_binder_batch(hname, psk_len, psk_type, shift):
    H, a = R.HLEN[hname], ALG[hname]
    for count in COUNTS:
        raw = prng_bytes(0x1700 + 7 * count + psk_len + 64 * psk_type, count * CONN)
        conns = _dev(raw, shift)
        want = [w["binder"] for w in _expected(hname, raw, count, psk_len, psk_type, 16)]
        oraw, wmatch = _offered(want, H, 0x1780 + count)
        offered = _dev(oraw, shift)
        bd, mt = Out(count, shift), Out(count, shift, el=4)
        K.batch_psk_binder(a, psk_len, psk_type, conns, offered, bd.view, mt.view, count)
        torch.cuda.synchronize()
        assert bd.read(H) == want, count
        assert mt.words() == wmatch, count
        # binders = NULL: the compare alone
        bd, mt = Out(count, shift), Out(count, shift, el=4)
        K.batch_psk_binder(a, psk_len, psk_type, conns, offered, None, mt.view, count)
        torch.cuda.synchronize()
        assert mt.words() == wmatch and bd.untouched(), count
        # a client computing its own binders: offered = match = NULL
        bd, mt = Out(count, shift), Out(count, shift, el=4)
        K.batch_psk_binder(a, psk_len, psk_type, conns, None, bd.view, None, count)
        torch.cuda.synchronize()
        assert bd.read(H) == want and mt.untouched(), count
        assert conns.cpu().numpy().tobytes() == raw and offered.cpu().numpy().tobytes() == oraw


# ---- the early keys ----------------------------------------------------------------------
def _slot_tuples(cipher, keys):
    return [(cipher, M.VERSION_TLS1_3, key, iv + bytes(4), 0) for key, iv in keys]


def _decrypt(kt, recs):
    d = B.Batch([], recs)
    out, res = d.run_gpu(True, kt=kt)
    return d, out, res


def _slots_decrypt(kt, cipher, keys, first, seed, neighbours=()):
    """slot first + i opens the record the oracle sealed under the checker's
    key / iv of connection i and rejects the record of connection i + 1;
    `neighbours`: (slot, key, iv) loaded before the call, which still open theirs"""
    slots = _slot_tuples(cipher, keys + [(k, iv) for _, k, iv in neighbours])
    lengths = [(53 * k + 1) % 300 for k in range(len(slots))]
    sealed, pre = B.sealed_records(slots, lengths, seed=seed)
    where = [first + i for i in range(len(keys))] + [s for s, _, _ in neighbours]
    for r in sealed:
        r.slot = where[r.slot]
    d, out, res = _decrypt(kt, sealed)
    for i, (r, p) in enumerate(zip(sealed, pre)):
        g = res[i]
        assert (int(g["status"]), int(g["data_len"]), int(g["type"])) == (0, p.data_len, p.type), i
        s0 = d.offs[i] + int(g["data_offset"])
        assert out[s0:s0 + p.data_len].tobytes() == bytes(p.buf[p.data_offset:p.data_offset + p.data_len]), i
    if len(keys) > 1:
        for i in range(len(keys) - 1):
            sealed[i + 1].slot = first + i
        _, _, res = _decrypt(kt, sealed[1:len(keys)])
        assert [int(g["status"]) for g in res] == [M.ERR_SSL_INVALID_MAC] * (len(keys) - 1)


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("psk_type", TYPES)
@pytest.mark.parametrize("psk_len", PSK_LENS)
@pytest.mark.parametrize("hname", HASHES)
def test_early_stage_outputs(hname, psk_len, psk_type, shift):
    """every output array against the checker; the keytab call gives the
    table-less call's binders; early_exporter = NULL is left alone"""
    H, a, cipher = R.HLEN[hname], ALG[hname], CIPHER[hname]
    kt = M.KeyTable(1 + 130)
    for count in (1, 65, 130):
        raw = prng_bytes(0x1800 + 7 * count + psk_len + 64 * psk_type, count * CONN)
        conns = _dev(raw, shift)
        want = _expected(hname, raw, count, psk_len, psk_type, M.KEYLEN[cipher])
        oraw, wmatch = _offered([w["binder"] for w in want], H, 0x1880 + count)
        offered = _dev(oraw, shift)
        ref = Out(count, shift)
        K.batch_psk_binder(a, psk_len, psk_type, conns, None, ref.view, None, count)
        for with_exp in (True, False):
            bd, mt, ce, ex = Out(count, shift), Out(count, shift, el=4), Out(count, shift), Out(count, shift)
            K.keytab_derive_early(kt, 1, count, cipher, psk_len, psk_type, conns, offered, bd.view, mt.view, ce.view,
                                  ex.view if with_exp else None)
            torch.cuda.synchronize()
            assert bd.read(H) == ref.read(H) == [w["binder"] for w in want], count
            assert mt.words() == wmatch, count
            assert ce.read(H) == [w["c_e"] for w in want], count
            if with_exp:
                assert ex.read(H) == [w["e_exp"] for w in want], count
            else:
                assert ex.untouched(), count
        assert conns.cpu().numpy().tobytes() == raw
    kt.close()


@pytest.mark.parametrize("cipher", [M.CIPHER_AES_128_GCM, M.CIPHER_AES_256_GCM, M.CIPHER_CHACHA20_POLY1305])
def test_early_slots_end_to_end(cipher):
    """the loaded slots open the checker's records and reject their neighbour's;
    the slots on both sides of the range keep the keys they held"""
    hname = HNAME[cipher]
    H, first = R.HLEN[hname], 3
    for count in (1, 65, 130):
        raw = prng_bytes(0x1900 + cipher + 16 * count, count * CONN)
        want = _expected(hname, raw, count, 32, K.PSK_RESUMPTION, M.KEYLEN[cipher])
        kt = M.KeyTable(first + count + 2)
        nb = [(s, prng_bytes(0x1990 + s, M.KEYLEN[cipher]), prng_bytes(0x19A0 + s, 12)) for s in (first - 1, first + count)]
        for s, key, iv in nb:
            kt.load(M.key_material(cipher, M.VERSION_TLS1_3, key, iv + bytes(4), 0), first=s)
        ce = Out(count)
        K.keytab_derive_early(kt, first, count, cipher, 32, K.PSK_RESUMPTION, _dev(raw), None, Out(count).view, None,
                              ce.view, None)
        torch.cuda.synchronize()
        assert ce.read(H) == [w["c_e"] for w in want]
        _slots_decrypt(kt, cipher, [w["keys"] for w in want], first, seed=61 + count, neighbours=nb)
        # the slots never loaded stay unloaded
        extra = B.plaintext_records([None], [40] * 3, seed=7)
        for r, s in zip(extra, (0, 1, first + count + 1)):
            r.slot = s
        _, eres = B.Batch([], extra).run_gpu(False, kt=kt)
        assert [int(r["status"]) for r in eres] == [BAD] * 3
        kt.close()


# ---- the ticket PSK ------------------------------------------------------------------------
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("nonce_len", [0, 1, 2, 8, 31, 32])
@pytest.mark.parametrize("hname", HASHES)
def test_ticket_psk(hname, nonce_len, shift):
    H, a = R.HLEN[hname], ALG[hname]
    for count in (1, 64, 65, 130):
        mraw = prng_bytes(0x1A00 + count + 256 * nonce_len, count * 48)
        nraw = bytearray(prng_bytes(0x1A80 + count + 256 * nonce_len, count * 32))
        want = [E.ticket_psk(hname, mraw[48 * i:48 * i + H], bytes(nraw[32 * i:32 * i + nonce_len])) for i in range(count)]
        for i in range(count):      # bytes past nonce_len must not change the result
            nraw[32 * i + nonce_len:32 * i + 32] = b"\xff" * (32 - nonce_len)
        rm, nonces, psk = _dev(mraw, shift), _dev(bytes(nraw), shift), Out(count, shift)
        K.batch_ticket_psk(a, nonce_len, rm, nonces, psk.view, count)
        torch.cuda.synchronize()
        assert psk.read(H) == want, count
        assert rm.cpu().numpy().tobytes() == mraw and nonces.cpu().numpy().tobytes() == bytes(nraw)


# ---- composition -------------------------------------------------------------------------
@pytest.mark.parametrize("hname", HASHES)
def test_composition_with_the_ladder_stages(hname):
    """application stage -> "res master" -> ticket PSK -> early stage under that
    PSK -> handshake stage under it: every value is the hashlib chain's, and the
    handshake stage gives what it gives without the early call before it"""
    H, a, cipher, count = R.HLEN[hname], ALG[hname], CIPHER[hname], 65
    kl = M.KEYLEN[cipher]
    mraw, t1, t2 = (prng_bytes(0x1B00 + k, count * 48) for k in range(3))
    nraw = prng_bytes(0x1B10, count * 32)
    hello = prng_bytes(0x1B20, count * 96)          # binder_transcript || hello_transcript
    rest = prng_bytes(0x1B30, count * 128)          # shared || transcript of the handshake stage
    first = 2
    kt, kt2 = M.KeyTable(first + 2 * count), M.KeyTable(first + 2 * count)
    ap, rm, psk = Out(2 * count), Out(count), Out(count)
    K.keytab_derive_application(kt, first, count, cipher, _dev(mraw), _dev(t1), ap.view, None)
    K.batch_derive_secret(a, b"res master", _dev(mraw), _dev(t2), rm.view, count)
    K.batch_ticket_psk(a, 32, rm.view, _dev(nraw), psk.view, count)
    torch.cuda.synchronize()
    masters = [mraw[48 * i:48 * i + H] for i in range(count)]
    w_ap = [R.application_stage(hname, masters[i], t1[48 * i:48 * i + H], kl) for i in range(count)]
    w_rm = [R.derive_secret(hname, masters[i], b"res master", t2[48 * i:48 * i + H]) for i in range(count)]
    w_psk = [E.ticket_psk(hname, w_rm[i], nraw[32 * i:32 * i + 32]) for i in range(count)]
    assert ap.read(H) == [w[k] for w in w_ap for k in ("c_ap", "s_ap")]
    assert rm.read(H) == w_rm and psk.read(H) == w_psk
    pskraw = psk.raw()
    early_conns = b"".join(pskraw[48 * i:48 * i + 48] + hello[96 * i:96 * i + 96] for i in range(count))
    hs_conns = b"".join(pskraw[48 * i:48 * i + 48] + rest[128 * i:128 * i + 128] for i in range(count))
    w_early = _expected(hname, early_conns, count, H, K.PSK_RESUMPTION, kl)
    oraw, wmatch = _offered([w["binder"] for w in w_early], H, 0x1B40)
    bd, mt, ce, ex = Out(count), Out(count, el=4), Out(count), Out(count)
    hs, fin, ms = Out(2 * count), Out(2 * count), Out(count)
    K.keytab_derive_early(kt, first, count, cipher, H, K.PSK_RESUMPTION, _dev(early_conns), _dev(oraw), bd.view, mt.view,
                          ce.view, ex.view)
    K.keytab_derive_handshake(kt, first, count, cipher, H, 32, _dev(hs_conns), hs.view, fin.view, ms.view)
    hs2, fin2, ms2 = Out(2 * count), Out(2 * count), Out(count)
    K.keytab_derive_handshake(kt2, first, count, cipher, H, 32, _dev(hs_conns), hs2.view, fin2.view, ms2.view)
    torch.cuda.synchronize()
    assert bd.read(H) == [w["binder"] for w in w_early] and mt.words() == wmatch
    assert ce.read(H) == [w["c_e"] for w in w_early] and ex.read(H) == [w["e_exp"] for w in w_early]
    w_hs = [R.handshake_stage(hname, w_psk[i], rest[128 * i:128 * i + 32], rest[128 * i + 80:128 * i + 80 + H], kl)
            for i in range(count)]
    assert hs.read(H) == hs2.read(H) == [w[k] for w in w_hs for k in ("c_hs", "s_hs")]
    assert fin.read(H) == fin2.read(H) == [w[k] for w in w_hs for k in ("c_fin", "s_fin")]
    assert ms.read(H) == ms2.read(H) == [w["master"] for w in w_hs]
    # the slot pairs of both tables hold the handshake keys: the same records under either
    slots = [(cipher, M.VERSION_TLS1_3, key, iv + bytes(4), 0) for w in w_hs for key, iv in (w["c_keys"], w["s_keys"])]
    recs = B.plaintext_records(slots, [(37 * k) % 200 for k in range(len(slots))], seed=71)
    for r in recs:
        r.slot += first
    got = [B.Batch([], recs).run_gpu(False, kt=t) for t in (kt, kt2)]
    want_out, want_res = B.Batch(_slot_tuples(cipher, [(bytes(kl), bytes(12))] * first) + slots, recs).run_gpu(False)
    assert [int(r["status"]) for r in want_res] == [0] * len(recs)
    for out, res in got:
        assert res.tobytes() == want_res.tobytes() and out.tobytes() == want_out.tobytes()
    kt.close()
    kt2.close()


# ---- arguments -------------------------------------------------------------------------------
def test_early_argument_errors_in_order():
    L = M.load()
    kt = M.KeyTable(9)
    c = M.CIPHER_AES_128_GCM
    conns = _dev(prng_bytes(1, 9 * CONN))
    o = Out(9)
    p, q, h = conns.data_ptr(), o.view.data_ptr(), kt.handle
    res = K.PSK_RESUMPTION
    ea = L.tlsrec_tls13_keytab_derive_early
    # BAD_INPUT_DATA wins over a cipher that would be FEATURE_UNAVAILABLE
    for cipher in (c, 0):
        assert ea(None, 0, 1, cipher, 32, res, p, q, q, q, q, q, None) == BAD
        assert ea(h, 0, 1, cipher, 32, res, None, q, q, q, q, q, None) == BAD       # conns
        assert ea(h, 0, 1, cipher, 32, res, p, q, q, q, None, q, None) == BAD       # early_traffic
        assert ea(h, 0, 1, cipher, 32, res, p, q, q, None, q, q, None) == BAD       # offered without match
        assert ea(h, 0, 1, cipher, 32, res, p, None, q, q, q, q, None) == BAD       # match without offered
        assert ea(h, 0, 0, cipher, 32, res, p, None, q, q, q, q, None) == BAD
        assert ea(h, 0, 1, cipher, 32, res, p, None, None, None, q, q, None) == BAD # neither binders nor match
        assert ea(h, 0, 1, cipher, 0, res, p, q, q, q, q, q, None) == BAD
        assert ea(h, 0, 1, cipher, 49, res, p, q, q, q, q, q, None) == BAD
        assert ea(h, 0, 0, cipher, 49, res, p, q, q, q, q, q, None) == BAD
        assert ea(h, 0, 10, cipher, 32, res, p, q, q, q, q, q, None) == BAD         # 10 slots in a table of 9
        assert ea(h, 5, 5, cipher, 32, res, p, q, q, q, q, q, None) == BAD
        assert ea(h, 10, 0, cipher, 32, res, p, q, q, q, q, q, None) == BAD
        assert ea(h, 1, 0xFFFFFFFF, cipher, 32, res, p, q, q, q, q, q, None) == BAD
    for cipher in (0, M.CIPHER_CAMELLIA_256_CCM + 1):
        assert ea(h, 0, 1, cipher, 32, res, p, q, q, q, q, q, None) == UNA
        assert ea(h, 0, 0, cipher, 32, res, p, q, q, q, q, q, None) == UNA          # before count == 0
    assert ea(h, 9, 0, c, 48, res, None, None, None, None, None, None, None) == 0
    assert ea(h, 0, 0, c, 1, 0, p, q, q, q, q, None, None) == 0
    torch.cuda.synchronize()
    # no refused call wrote anything or loaded a slot
    assert o.untouched()
    extra = B.plaintext_records([None], [40] * 9, seed=2)
    for s, r in enumerate(extra):
        r.slot = s
    _, eres = B.Batch([], extra).run_gpu(False, kt=kt)
    assert [int(r["status"]) for r in eres] == [BAD] * 9
    kt.close()
