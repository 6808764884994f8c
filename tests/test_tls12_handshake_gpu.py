"""GPU parity of the TLS 1.2 / DTLS 1.2 handshake batches (tls12_batch.hip, through
the C ABI): tlsrec_tls12_batch_compute_master and tlsrec_tls12_batch_verify_data
against the checker of tests/tls12_hs_ref.py (P_hash over hashlib, cross-checked
by OpenSSL's TLS1-PRF) -- every output byte bit-exact over the premaster lengths
at which the key block, the key hash and its padding change shape, at the
workgroup edges, aligned and 4 bytes off; the Finished compare on offered values
wrong in their first bit, their last bit or only past byte 11; the single-shot
calls against the batches; and the chain master -> key expansion -> records on
one stream, checked by the record paths of the key-derivation tests."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

import mbedtls_amd as M  # noqa: E402
from mbedtls_amd import tls12 as T  # noqa: E402
from tests import cbc_ref as R  # noqa: E402
from tests import test_tls12_cbc_derive_gpu as CG  # noqa: E402  (its record checks for CBC slots)
from tests import test_tls12_keys_gpu as KG  # noqa: E402  (its record checks and DTLS exchange)
from tests import tls12_hs_ref as H  # noqa: E402
from tests.prng import prng_bytes  # noqa: E402
from tests.test_tls13_early_gpu import Out, _dev  # noqa: E402  (guarded device arrays)

PRF = {"sha256": T.PRF_SHA256, "sha384": T.PRF_SHA384}
PRFS = sorted(PRF)
# 55 / 56: the SHA-256 key fits its block with room to spare; 63 / 64 / 65: the key fills the block, then is hashed;
# 118 / 119 / 120: the key hash's padding takes a third block from 120; 127 / 128: the last byte, a 0x80 on a block start
PMS_LENS = [1, 32, 48, 55, 56, 63, 64, 65, 66, 118, 119, 120, 127, 128]
COUNTS = [1, 63, 64, 65, 130]           # one lane per connection, 64 per workgroup
SHIFTS = [0, 4]                         # every array 16-byte aligned / 4 bytes off (the byte paths)
BAD, UNA = M.ERR_SSL_BAD_INPUT_DATA, M.ERR_SSL_FEATURE_UNAVAILABLE
PC, CN = H.PMS_CONN, H.CONN


def _pms_conns(seed, count, pms_len, hname):
    """count tlsrec_tls12_pms_conn; every byte the call must not look at is 0xFF, so a missing mask fails"""
    raw = bytearray(prng_bytes(seed, count * PC))
    hl = H.HLEN[hname]
    for i in range(count):
        raw[PC * i + pms_len:PC * i + 128] = b"\xff" * (128 - pms_len)
        raw[PC * i + 192 + hl:PC * i + 240] = b"\xff" * (48 - hl)
    return bytes(raw)


def _want_conns(hname, raw, count, pms_len, ems):
    return b"".join(H.conn_out(hname, raw[PC * i:PC * i + PC], pms_len, ems) for i in range(count))


# ---- the master secret ---------------------------------------------------------------
@pytest.mark.parametrize("ems", [0, 1])
@pytest.mark.parametrize("hname", PRFS)
def test_master_over_premaster_lengths(hname, ems):
    count = 65
    for pms_len in PMS_LENS:
        raw = _pms_conns(0x2100 + 2 * pms_len + ems, count, pms_len, hname)
        conns, out = _dev(raw), Out(count, el=CN)
        T.tls12_batch_compute_master(PRF[hname], pms_len, ems, conns, out.view, count)
        torch.cuda.synchronize()
        got, want = out.raw(), _want_conns(hname, raw, count, pms_len, bool(ems))
        for i in range(count):
            assert got[CN * i:CN * i + 48] == want[CN * i:CN * i + 48], (pms_len, i, "master")
            assert got[CN * i + 48:CN * i + 80] == raw[PC * i + 160:PC * i + 192], (pms_len, i, "server_random")
            assert got[CN * i + 80:CN * i + 112] == raw[PC * i + 128:PC * i + 160], (pms_len, i, "client_random")
        assert got == want and conns.cpu().numpy().tobytes() == raw, pms_len


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("hname", PRFS)
def test_master_workgroup_edges(hname, shift):
    for count in COUNTS:
        for pms_len in (48, 66):
            for ems in (0, 1):
                raw = _pms_conns(0x2200 + 8 * count + pms_len + ems, count, pms_len, hname)
                conns, out = _dev(raw, shift), Out(count, shift, el=CN)
                T.tls12_batch_compute_master(PRF[hname], pms_len, ems, conns, out.view, count)
                torch.cuda.synchronize()
                assert out.raw() == _want_conns(hname, raw, count, pms_len, bool(ems)), (count, pms_len, ems)
                assert conns.cpu().numpy().tobytes() == raw


@pytest.mark.parametrize("hname", PRFS)
def test_master_agrees_with_the_single_shot_call(hname):
    count, hl = 4, H.HLEN[hname]
    for pms_len in (32, 66, 128):
        for ems in (0, 1):
            raw = _pms_conns(0x2300 + pms_len + ems, count, pms_len, hname)
            out = Out(count, el=CN)
            T.tls12_batch_compute_master(PRF[hname], pms_len, ems, _dev(raw), out.view, count)
            torch.cuda.synchronize()
            got = out.raw()
            for i in range(count):
                c = raw[PC * i:PC * i + PC]
                seed = c[192:192 + hl] if ems else c[128:192]
                assert T.tls12_compute_master(PRF[hname], c[:pms_len], seed, bool(ems)) == got[CN * i:CN * i + 48]


def test_master_refused_calls_launch_nothing():
    """count == 0, and the FFDH length: pms_len == 129 is FEATURE_UNAVAILABLE; `out` keeps its bytes"""
    fn = M.load().tlsrec_tls12_batch_compute_master
    conns, out = _dev(_pms_conns(0x2400, 4, 48, "sha256")), Out(4, el=CN)
    for prf in PRF.values():
        assert fn(prf, 129, 0, conns.data_ptr(), out.view.data_ptr(), 4, None) == UNA
        assert fn(prf, 0, 1, conns.data_ptr(), out.view.data_ptr(), 4, None) == BAD
        assert fn(prf, 48, 0, conns.data_ptr(), out.view.data_ptr(), 0, None) == 0
        assert fn(prf, 128, 1, None, None, 0, None) == 0
    assert fn(T.PRF_NONE, 48, 0, conns.data_ptr(), out.view.data_ptr(), 4, None) == UNA
    with pytest.raises(T.KeyScheduleError) as e:
        T.tls12_batch_compute_master(T.PRF_SHA384, 129, True, conns, out.view, 4)
    assert e.value.code == UNA
    torch.cuda.synchronize()
    assert out.untouched()


# ---- Finished ------------------------------------------------------------------------
def _transcripts(seed, count, hname):
    hl = H.HLEN[hname]
    raw = bytearray(prng_bytes(seed, 48 * count))
    for i in range(count):
        raw[48 * i + hl:48 * i + 48] = b"\xff" * (48 - hl)
    return bytes(raw)


def _offered(values, seed):
    """16-byte offered elements and the match vector they must give: the right value, except i % 5 == 2 (the
    first bit wrong), i % 5 == 4 (the last bit of byte 11 wrong) and i % 5 == 0 (only bytes 12..15 differ from
    what `verify` receives: still a match)"""
    raw, want = bytearray(), []
    for i, v in enumerate(values):
        o, ok = bytearray(v + bytes(4)), 1
        if i % 5 == 2:
            o[0] ^= 0x80
            ok = 0
        elif i % 5 == 4:
            o[11] ^= 0x01
            ok = 0
        elif i % 5 == 0:
            o[12:] = bytes(x | 1 for x in prng_bytes(seed + i, 4))
        raw += o
        want.append(ok)
    return bytes(raw), want


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("frm", [T.IS_CLIENT, T.IS_SERVER])
@pytest.mark.parametrize("hname", PRFS)
def test_verify_data_batch(hname, frm, shift):
    hl, prf = H.HLEN[hname], PRF[hname]
    fn = M.load().tlsrec_tls12_batch_verify_data
    for count in COUNTS:
        raw = prng_bytes(0x2500 + 4 * count + frm, CN * count)
        traw = _transcripts(0x2580 + count, count, hname)
        want = [H.verify_data(hname, raw[CN * i:CN * i + 48], traw[48 * i:48 * i + hl], frm) for i in range(count)]
        oraw, wmatch = _offered(want, 0x25C0 + count)
        assert count < 5 or {0, 1} == set(wmatch)
        conns, trs, offered = _dev(raw, shift), _dev(traw, shift), _dev(oraw, shift)
        vd, mt = Out(count, shift, el=16), Out(count, shift, el=4)
        T.tls12_batch_verify_data(prf, frm, conns, trs, offered, vd.view, mt.view, count)
        torch.cuda.synchronize()
        assert vd.raw() == b"".join(w + bytes(4) for w in want), count
        assert mt.words() == wmatch, count
        # verify = NULL: the compare alone
        vd, mt = Out(count, shift, el=16), Out(count, shift, el=4)
        T.tls12_batch_verify_data(prf, frm, conns, trs, offered, None, mt.view, count)
        torch.cuda.synchronize()
        assert mt.words() == wmatch and vd.untouched(), count
        # an endpoint computing its own Finished: offered = match = NULL
        vd, mt = Out(count, shift, el=16), Out(count, shift, el=4)
        T.tls12_batch_verify_data(prf, frm, conns, trs, None, vd.view, None, count)
        torch.cuda.synchronize()
        assert vd.raw() == b"".join(w + bytes(4) for w in want) and mt.untouched(), count
        # refused calls write nothing
        vd, mt = Out(count, shift, el=16), Out(count, shift, el=4)
        p = [x.data_ptr() for x in (conns, trs, offered, vd.view, mt.view)]
        assert fn(prf, 2, *p, count, None) == BAD
        assert fn(T.PRF_NONE, frm, *p, count, None) == UNA
        assert fn(prf, frm, p[0], p[1], p[2], p[3], None, count, None) == BAD
        assert fn(prf, frm, p[0], p[1], None, p[3], p[4], count, None) == BAD
        assert fn(prf, frm, None, p[1], p[2], p[3], p[4], count, None) == BAD
        assert fn(prf, frm, p[0], p[1], p[2], p[3], p[4], 0, None) == 0
        torch.cuda.synchronize()
        assert vd.untouched() and mt.untouched(), count
        for x, r in ((conns, raw), (trs, traw), (offered, oraw)):
            assert x.cpu().numpy().tobytes() == r
        # the single-shot call
        for i in sorted({0, count // 2, count - 1}):
            assert T.tls12_calc_finished(prf, raw[CN * i:CN * i + 48], traw[48 * i:48 * i + hl], frm) == want[i]


# ---- master -> key expansion -> records, on one stream ---------------------------------
def _chain(hname, pms_len, ems, count, seed, derive):
    """batch_compute_master, `derive(out)` and both Finished batches from the same `out`, enqueued back to back;
    returns the checker's tlsrec_tls12_conn array after checking `out` and the Finished values against it"""
    hl, prf = H.HLEN[hname], PRF[hname]
    raw = _pms_conns(seed, count, pms_len, hname)
    traw = [_transcripts(seed + 1 + k, count, hname) for k in (0, 1)]
    conns, out = _dev(raw), Out(count, el=CN)
    trs = [_dev(t) for t in traw]
    vds = [Out(count, el=16), Out(count, el=16)]
    T.tls12_batch_compute_master(prf, pms_len, ems, conns, out.view, count)
    derive(out.view)
    for frm in (T.IS_CLIENT, T.IS_SERVER):
        T.tls12_batch_verify_data(prf, frm, out.view, trs[frm], None, vds[frm].view, None, count)
    torch.cuda.synchronize()
    want = _want_conns(hname, raw, count, pms_len, bool(ems))
    assert out.raw() == want
    for frm in (T.IS_CLIENT, T.IS_SERVER):
        assert vds[frm].raw() == b"".join(
            H.verify_data(hname, want[CN * i:CN * i + 48], traw[frm][48 * i:48 * i + hl], frm) + bytes(4)
            for i in range(count))
    return want


@pytest.mark.parametrize("hname,cipher,pms_len,ems", [("sha256", M.CIPHER_AES_128_GCM, 32, 1),
                                                      ("sha384", M.CIPHER_AES_256_GCM, 66, 0)])
def test_chain_into_aead_slots(hname, cipher, pms_len, ems):
    """the derived table encrypts TLS 1.2 records as the oracle's record layer does under the checker's keys,
    and a client's and a server's table derived from the same `out` exchange DTLS 1.2 datagrams"""
    count, first = 65, 3
    tabs = {ep: M.KeyTable(first + 2 * count + 2) for ep in (T.IS_CLIENT, T.IS_SERVER)}

    def derive(out):
        for kt in tabs.values():
            T.tls12_keytab_derive(kt, first, count, cipher, PRF[hname], out)

    want = _chain(hname, pms_len, ems, count, 0x2600 + pms_len, derive)
    slots = KG._expected_slots(hname, cipher, want, count)
    lengths = [(37 * k) % 300 for k in range(2 * count)]
    KG._check_records(tabs[T.IS_SERVER], slots, first, lengths, seed=23,
                      unloaded=[0, 1, 2, first + 2 * count, first + 2 * count + 1])
    nconn = 4
    for sender, receiver in ((T.IS_CLIENT, T.IS_SERVER), (T.IS_SERVER, T.IS_CLIENT)):
        jobs, pts = [], []
        for i in range(nconn):
            enc, _ = T.tls12_slots(first, i, sender)
            pts.append([prng_bytes(0x2680 + 16 * i + k + 64 * sender, (1, 200, 1400)[k]) for k in range(3)])
            for k in range(3):
                jobs.append((enc, pts[i][k], (1).to_bytes(2, "big") + (5 * i + k).to_bytes(6, "big")))
        grams = KG._dtls_send(tabs[sender], jobs)
        rx = [(T.tls12_slots(first, i, receiver)[1], grams[3 * i:3 * (i + 1)]) for i in range(nconn)]
        assert KG._dtls_receive(tabs[receiver], rx) == pts
    for kt in tabs.values():
        kt.close()


@pytest.mark.parametrize("etm", [0, 1])
def test_chain_into_cbc_slots(etm):
    """the same through tlsrec_tls12_keytab_derive_cbc for AES-128-CBC + HMAC-SHA256: records sealed by the
    table match the CBC record model under the checker's keys, and the model's records open"""
    count, first, hname = 65, 3, "sha256"
    cipher, mac = R.CIPHER_AES_128_CBC, R.MAC_SHA256
    kt = M.KeyTable(first + 2 * count + 2)
    want = _chain(hname, 48, etm, count, 0x2700 + etm,
                  lambda out: T.tls12_keytab_derive_cbc(kt, first, count, cipher, mac, etm, PRF[hname], out))
    slots = [None] * first + CG._expected_keys(hname, cipher, mac, etm, want, count) + [None] * 2
    CG._check_records(kt, slots, [(37 * k) % 300 for k in range(2 * count)], seed=29,
                      unloaded=[0, first + 2 * count])
    kt.close()
