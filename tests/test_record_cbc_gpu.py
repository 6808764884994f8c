"""CBC + HMAC transforms through the single-record calls (tlsrec_transform_setup_cbc,
tlsrec_encrypt_buf / tlsrec_decrypt_buf) on the GPU, bit-exact against the models of
tests/cbc_ref.py and tests/cbc_alt_ref.py (hashlib + OpenSSL): every suite in both MAC
orders, the edges of the wave-per-record decryption kernel and the lane kernel behind
TLSREC_CBC_WAVE=0, the padding / MAC sweep across the wave's round boundaries, the framing
statuses, DTLS 1.2 connection IDs, fail-closed, zeroization and the engine's CBC queues."""
from __future__ import annotations

import ctypes
import threading

import numpy as np
import pytest

import mbedtls_amd as M
import oracle as O
from mbedtls_amd import _abi
from tests import cbc_alt_ref as A
from tests import cbc_ref as R
from tests.batchlib import launch_log  # noqa: F401  (fixture)
from tests.prng import prng_bytes

pytestmark = pytest.mark.gpu

AES_SUITES = [(c, m) for c in (R.CIPHER_AES_128_CBC, R.CIPHER_AES_256_CBC) for m in (R.MAC_SHA1, R.MAC_SHA256, R.MAC_SHA384)]
SUITES = AES_SUITES + list(A.SUITES)
PIN_IV = bytes(range(0xA0, 0xB0))
TLS, DTLS = b"\x03\x03", b"\xfe\xfd"


def _sid(p):
    return "-".join(str(x) for x in p) if isinstance(p, tuple) else str(p)


class Conn:
    """a CBC transform and the model's keys of its two directions (different keys each way)"""

    def __init__(self, cipher, mac, etm, seed, in_cid=b"", out_cid=b""):
        kl, ml = A.ALL_KEYLEN[cipher], R.MACLEN[mac]
        b = prng_bytes(seed, 4 * 48)
        ke, kd, me, md = b[0:kl], b[48:48 + kl], b[96:96 + ml], b[144:144 + ml]
        self.t = M.Transform.cbc(M.VERSION_TLS1_2, cipher, mac, etm, ke, kd, me, md)
        if in_cid or out_cid:
            self.t.set_cid(in_cid, out_cid)
        self.enc = R.Key(cipher, mac, etm, ke, me, out_cid)
        self.dec = R.Key(cipher, mac, etm, kd, md, in_cid)
        self.mac, self.etm, self.maclen = mac, etm, ml
        self.st = None                   # the status of the last call

    def close(self):
        self.t.close()

    def encrypt(self, buf, off, ln, ctr, rtype=23, ver=TLS, buf_len=None, iv=PIN_IV):
        """-> mismatches against the model (empty = exact), the record after the call.  The model is
        given `iv` in front of the content; the call is given other bytes there."""
        buf_len = len(buf) if buf_len is None else buf_len
        mbuf = bytearray(buf[:buf_len])
        if off >= 16 and off <= buf_len:
            mbuf[off - 16:off] = iv
        want = A.encrypt(self.enc, bytes(mbuf), off, ln, ctr, rtype, ver)
        rec = M.Record(ctr=ctr, type=rtype, ver=ver, buf=bytearray(buf), data_offset=off, data_len=ln, buf_len=buf_len)
        st = self.st = self.t.encrypt_buf(rec)
        bad = _diff(st, rec, want, buf_len)
        if want.cid_len and rec.cid != self.enc.cid:
            bad.append(f"cid {rec.cid.hex()} != {self.enc.cid.hex()}")
        return bad, rec

    def decrypt(self, buf, off, ln, ctr, rtype=23, ver=TLS, cid=b"", buf_len=None):
        buf_len = len(buf) if buf_len is None else buf_len
        want = A.decrypt(self.dec, bytes(buf[:buf_len]), off, ln, ctr, rtype, ver, cid)
        rec = M.Record(ctr=ctr, type=rtype, ver=ver, buf=bytearray(buf), data_offset=off, data_len=ln, buf_len=buf_len,
                       cid=cid)
        st = self.st = self.t.decrypt_buf(rec)
        return _diff(st, rec, want, buf_len), rec

    def seal(self, content, ctr, rtype=23, ver=TLS, iv=PIN_IV, tail=96):
        """the model's encryption under the key this transform DECRYPTS with -> (buf, off, len, type)"""
        buf = iv + content + bytes(96 if tail is None else tail)      # tail None: the record ends its buffer
        e = A.encrypt(self.dec, buf, 16, len(content), ctr, rtype, ver)
        assert e.status == 0
        return bytearray(e.buf[:e.data_offset + e.data_len] if tail is None else e.buf), e.data_offset, e.data_len, e.type


def _diff(st, rec, want, buf_len):
    got = (st, rec.data_offset, rec.data_len, rec.type)
    exp = (want.status, want.data_offset, want.data_len, want.type)
    if got != exp:
        return [f"fields {got} != {exp}"]
    if st == 0 and bytes(rec.buf[:buf_len]) != want.buf:      # the bytes of a failed record are unspecified
        j = next(j for j in range(buf_len) if rec.buf[j] != want.buf[j])
        return [f"bytes differ from {j}"]
    return []


@pytest.fixture
def hooks():
    """the test-hooks library with the explicit IV pinned"""
    with _abi.use_library() as lib:
        pin = lib.tlsrec__test_pin_cbc_iv
        pin.argtypes, pin.restype = [ctypes.c_char_p], None
        pin(PIN_IV)
        try:
            yield lib
        finally:
            pin(None)


def _plain(n, seed, head=16, tail=96):
    return bytearray(b"\xee" * head) + bytearray(prng_bytes(seed, n)) + bytearray(tail)


@pytest.mark.parametrize("etm", [0, 1])
@pytest.mark.parametrize("suite", SUITES, ids=_sid)
def test_round_trip_and_known_answers(hooks, suite, etm):
    c = Conn(*suite, etm, 1000 + 10 * suite[0] + suite[1])
    try:
        for i, n in enumerate((0, 1, 15, 16, 17, 100, 1400)):
            ctr = prng_bytes(50 + i, 8)
            bad, rec = c.encrypt(_plain(n, 7 * n + etm), 16, n, ctr)
            assert not bad, ("encrypt", n, bad)
            assert bytes(rec.buf[0:16]) == PIN_IV and rec.data_offset == 0
            content = prng_bytes(9 * n + 1, n)
            buf, off, ln, rtype = c.seal(content, ctr)
            bad, rec = c.decrypt(buf, off, ln, ctr, rtype)
            assert not bad, ("decrypt", n, bad)
            assert rec.data() == content
    finally:
        c.close()


def test_release_library_draws_the_iv():
    """no hook: the IV in the output is the one the record was encrypted under, and two
    encryptions of one record draw different IVs"""
    c = Conn(R.CIPHER_AES_128_CBC, R.MAC_SHA256, 0, 77)
    try:
        ctr, outs = bytes(8), []
        for _ in range(2):
            rec = M.Record(ctr=ctr, type=23, ver=TLS, buf=_plain(333, 5), data_offset=16, data_len=333)
            assert c.t.encrypt_buf(rec) == 0
            iv = bytes(rec.buf[0:16])
            want = A.encrypt(c.enc, iv + bytes(_plain(333, 5)[16:]), 16, 333, ctr, 23, TLS)
            assert (rec.data_offset, rec.data_len, bytes(rec.buf)) == (want.data_offset, want.data_len, want.buf)
            outs.append(iv)
        assert outs[0] != outs[1] and outs[0] != b"\xee" * 16
    finally:
        c.close()


def _content_for_blocks(nblk, maclen, etm):
    """content length whose ciphertext (after the IV) is nblk blocks, padding of one byte"""
    return 16 * nblk - 1 - (0 if etm else maclen)


@pytest.mark.parametrize("etm", [0, 1])
@pytest.mark.parametrize("suite", [(R.CIPHER_AES_128_CBC, R.MAC_SHA1), (R.CIPHER_AES_128_CBC, R.MAC_SHA256),
                                   (R.CIPHER_AES_256_CBC, R.MAC_SHA384), A.SUITES[0], A.SUITES[-1]], ids=_sid)
def test_wave_kernel_edges(launch_log, monkeypatch, suite, etm):  # noqa: F811
    """ciphertext block counts at the suite's minimum, around one and two rounds of the wave
    and at the largest record; the wave kernel by default, the lane kernel with
    TLSREC_CBC_WAVE=0, identical results"""
    c = Conn(*suite, etm, 2000 + suite[0])
    try:
        lens = [0] + [_content_for_blocks(b, c.maclen, etm) for b in (63, 64, 65, 127, 128, 129)] + [16384]
        blocks = {2: R.MAC_SHA1, 3: R.MAC_SHA256, 4: R.MAC_SHA384}
        sealed = []
        for i, n in enumerate(lens):
            ctr = prng_bytes(300 + i, 8)
            buf, off, ln, rtype = c.seal(prng_bytes(11 * i + 3, n), ctr, tail=None)
            sealed.append((buf, off, ln, ctr, rtype, n))
        nblk0 = (sealed[0][2] - 16 - (c.maclen if etm else 0)) // 16
        assert nblk0 == 1 if etm else blocks[nblk0] == c.mac           # the suite's minimum
        assert [(s[2] - 16 - (c.maclen if etm else 0)) // 16 for s in sealed[1:7]] == [63, 64, 65, 127, 128, 129]
        got = {}
        for knob, kernel in ((None, 1), ("0", 0)):
            if knob is not None:
                monkeypatch.setenv("TLSREC_CBC_WAVE", knob)
            launch_log.reset()
            outs = []
            for buf, off, ln, ctr, rtype, n in sealed:
                bad, rec = c.decrypt(buf, off, ln, ctr, rtype)
                assert not bad, (knob, n, bad)
                assert rec.data_len == n
                outs.append((rec.data_offset, rec.data_len, rec.type, bytes(rec.buf)))
            got[kernel] = outs
            log = launch_log(_abi.LOG_CBC_KERNEL)
            assert len(log) == len(sealed) and all(e[1] == kernel and e[2] == 1 for e in log), log[:3]
        assert got[0] == got[1]
    finally:
        c.close()


def _pre(c, ctr, content_len, padlen, fill=42):
    """plaintext || MAC || padding of a MAC-then-encrypt record, before encryption"""
    data = bytes([fill]) * content_len
    return data + R._mac(c.dec, ctr, 23, TLS, data, b"") + bytes([padlen]) * (padlen + 1)


def _seal_pre(c, pre):
    return bytearray(PIN_IV + A.block_cbc(c.dec.cipher, c.dec.key, PIN_IV, pre, True))


@pytest.mark.parametrize("nblk", [65, 129])
def test_padding_and_mac_sweep(hooks, nblk):
    """MAC-then-encrypt decryption where padding and MAC straddle a round boundary of the
    wave: every pad length, wrong pad bytes, a flipped MAC byte, a pad length too large"""
    c = Conn(R.CIPHER_AES_128_CBC, R.MAC_SHA256, 0, 31)
    ctr = bytes(8)
    try:
        cases = []                                     # (plaintext before encryption, expected status)
        for padlen in range(256):                      # every pad length fits: 16 nblk > 32 + 256
            cases.append((_pre(c, ctr, 16 * nblk - 32 - padlen - 1, padlen), 0))
        for padlen in (1, 15, 16, 17, 255):
            pre = cases[padlen][0]
            for pos in (len(pre) - padlen - 1, len(pre) - padlen // 2 - 1, len(pre) - 1):     # first, middle, last
                b = bytearray(pre)
                b[pos] ^= 0x01
                cases.append((bytes(b), M.ERR_SSL_INVALID_MAC))
        pre = bytearray(cases[40][0])
        pre[len(pre) - 41 - 32] ^= 0x80                # first MAC byte
        cases.append((bytes(pre), M.ERR_SSL_INVALID_MAC))
        pre = bytearray(cases[3][0])
        pre[-1] = 255                                  # claims 255 bytes of padding, has 3
        cases.append((bytes(pre), M.ERR_SSL_INVALID_MAC))
        for pre, status in cases:
            buf = _seal_pre(c, pre)
            want = A.decrypt(c.dec, bytes(buf), 0, len(buf), ctr, 23, TLS)
            assert want.status == status               # the model agrees with the construction
            bad, _ = c.decrypt(buf, 0, len(buf), ctr)
            assert not bad, (len(pre), status, bad)
        # a pad length larger than the record: 3 blocks, last byte 255
        pre = bytearray(_pre(c, ctr, 15, 0))
        pre[-1] = 255
        buf = _seal_pre(c, bytes(pre))
        bad, rec = c.decrypt(buf, 0, len(buf), ctr)
        assert not bad and rec.data_len == 48 - 32, bad
    finally:
        c.close()


@pytest.mark.parametrize("nblk", [65, 129])
def test_encrypt_then_mac_tampering(hooks, nblk):
    """a flipped IV, ciphertext or MAC byte: INVALID_MAC, and no byte of the record written"""
    c = Conn(R.CIPHER_AES_256_CBC, R.MAC_SHA384, 1, 32)
    ctr = prng_bytes(8, 8)
    try:
        buf, off, ln, rtype = c.seal(prng_bytes(1, _content_for_blocks(nblk, 48, 1)), ctr)
        for pos in (0, 15, 16, 16 + 16 * 63 + 5, 16 + 16 * 64, ln - 48 - 1, ln - 48, ln - 1):
            b = bytearray(buf)
            b[pos] ^= 0x10
            bad, rec = c.decrypt(b, off, ln, ctr, rtype)
            assert not bad, (pos, bad)
            assert (rec.data_offset, rec.data_len) == (0, ln - 48)
            assert bytes(rec.buf) == bytes(b), f"flip at {pos}: the record was written before the MAC check"
    finally:
        c.close()


@pytest.mark.parametrize("etm", [0, 1])
def test_framing_statuses(hooks, etm):
    c = Conn(R.CIPHER_AES_128_CBC, R.MAC_SHA256, etm, 33)
    ctr = bytes(8)
    seen = set()
    try:
        # encrypt: every amount of room behind the content, short heads, too long a record
        for n in (0, 5, 31):
            for room in range(0, 16 + 32 + 2):
                bad, rec = c.encrypt(_plain(n, n, tail=room), 16, n, ctr)
                assert not bad, ("room", n, room, bad)
                seen.add(c.st)
            for head in (0, 8, 15):
                bad, _ = c.encrypt(_plain(n, n, head=head), head, n, ctr)
                assert not bad, ("head", n, head, bad)
        assert seen == {0, M.ERR_SSL_BUFFER_TOO_SMALL}
        bad, rec = c.encrypt(_plain(16385, 1, tail=128), 16, 16385, ctr)
        assert not bad and rec.data_len == 16385, bad
        buf = _plain(100, 2)
        bad, rec = c.encrypt(buf, 16, 100, ctr, buf_len=115)         # the content runs past the buffer
        assert not bad, bad
        bad, rec = c.encrypt(buf, len(buf) + 1, 0, ctr)
        assert not bad, bad
        # decrypt: below minlen, not a block multiple, past the buffer
        buf, off, ln, rtype = c.seal(prng_bytes(3, 40), ctr)
        minlen = R.minlen(R.MAC_SHA256, etm)
        assert int(c.t._t.minlen) == minlen
        for n in sorted({0, 1, 16, 31, 32, 48, 49, minlen - 1, minlen, ln - 16, ln - 15, ln - 1, ln}):
            bad, _ = c.decrypt(buf, off, n, ctr, rtype)
            assert not bad, ("len", n, bad)
        bad, _ = c.decrypt(buf, off, ln, ctr, rtype, buf_len=ln - 1)
        assert not bad, bad
        bad, _ = c.decrypt(buf, 8, len(buf) - 4, ctr, rtype)
        assert not bad, bad
    finally:
        c.close()


@pytest.mark.parametrize("etm", [0, 1])
def test_dtls12_with_and_without_cid(hooks, etm):
    cid_in, cid_out = bytes(range(0x10, 0x15)), bytes(range(0x40, 0x60))
    ctr = (1).to_bytes(2, "big") + (1000).to_bytes(6, "big")
    for in_cid, out_cid in ((b"", b""), (cid_in, cid_out)):
        c = Conn(R.CIPHER_AES_256_CBC, R.MAC_SHA1, etm, 34, in_cid, out_cid)
        try:
            for n in (0, 1, 15, 16, 100, 1400):
                bad, rec = c.encrypt(_plain(n, n, tail=128), 16, n, ctr, ver=DTLS)
                assert not bad, (n, bad)
                assert rec.type == (M.MSG_CID if out_cid else 23)
                content = prng_bytes(n + 9, n)
                e = A.encrypt(c.dec, PIN_IV + content + bytes(128), 16, n, ctr, 23, DTLS)
                bad, rec = c.decrypt(bytearray(e.buf), e.data_offset, e.data_len, ctr, e.type, DTLS, cid=in_cid)
                assert not bad, (n, bad)
                assert (rec.type, rec.data()) == (23, content)
            # a record with another CID, with none where one is expected, with one where none is
            e = A.encrypt(c.dec, PIN_IV + bytes(50) + bytes(128), 16, 50, ctr, 23, DTLS)
            for other in ((b"\x10\x11\x12\x13\x99", b"") if in_cid else (cid_in,)):
                bad, rec = c.decrypt(bytearray(e.buf), e.data_offset, e.data_len, ctr, e.type, DTLS, cid=other)
                assert not bad, bad
                assert c.st == M.ERR_SSL_UNEXPECTED_CID
            if in_cid:
                # an inner plaintext of zeros only, sealed by hand
                inner = bytes(16)
                if etm:
                    body = inner + bytes([15]) * 16
                    ct = PIN_IV + A.block_cbc(c.dec.cipher, c.dec.key, PIN_IV, body, True)
                    wire = ct + R._mac(c.dec, ctr, M.MSG_CID, DTLS, ct, in_cid)
                else:
                    body = inner + R._mac(c.dec, ctr, M.MSG_CID, DTLS, inner, in_cid)
                    padlen = 15 - len(body) % 16
                    body += bytes([padlen]) * (padlen + 1)
                    wire = PIN_IV + A.block_cbc(c.dec.cipher, c.dec.key, PIN_IV, body, True)
                bad, rec = c.decrypt(bytearray(wire), 0, len(wire), ctr, M.MSG_CID, DTLS, cid=in_cid)
                assert not bad, bad
                assert c.st == M.ERR_SSL_INVALID_RECORD
        finally:
            c.close()


def test_unreached_record_fails_closed(hooks):
    """the skip hook: INTERNAL_ERROR, the record and its buffer as given"""
    skip = hooks.tlsrec__test_skip_record
    skip.argtypes, skip.restype = [ctypes.c_uint32], None
    for etm in (0, 1):
        c = Conn(R.CIPHER_AES_128_CBC, R.MAC_SHA256, etm, 35)
        try:
            ctr = bytes(8)
            sealed, off, ln, rtype = c.seal(prng_bytes(2, 1400), ctr)
            skip(0)
            for decrypt, buf, o, n in ((False, _plain(1400, 3), 16, 1400), (True, sealed, off, ln)):
                rec = M.Record(ctr=ctr, type=23, ver=TLS, buf=bytearray(buf), data_offset=o, data_len=n)
                st = (c.t.decrypt_buf if decrypt else c.t.encrypt_buf)(rec)
                assert st == M.ERR_SSL_INTERNAL_ERROR
                assert (rec.data_offset, rec.data_len, rec.type, bytes(rec.buf)) == (o, n, 23, bytes(buf))
            skip(0xFFFFFFFF)
            bad, _ = c.decrypt(sealed, off, ln, ctr, rtype)
            assert not bad, bad
        finally:
            skip(0xFFFFFFFF)
            c.close()


@pytest.mark.parametrize("suite", [(R.CIPHER_AES_256_CBC, R.MAC_SHA384), A.SUITES[1]], ids=_sid)
def test_transform_free_zeroizes_device_slots(hooks, suite):
    dump = hooks.tlsrec__test_engine_slot_dump
    dump.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    c = Conn(*suite, 0, 36)
    slots = (int(c.t._t.slot_enc), int(c.t._t.slot_dec))
    bufs = [np.zeros(1024, np.uint8) for _ in range(3)]

    def snap(s):
        assert dump(s, *(b.ctypes.data for b in bufs)) == 0
        return [b.copy() for b in bufs]

    for s in slots:
        st, gh, _ = snap(s)
        assert st[64:544].any() and st[600:872].any()         # SlotState rk / rkr and ark: round keys of both directions
        assert gh[:128].any()                                 # the HMAC midstates
    c.close()
    for s in slots:
        st, gh, hp = snap(s)
        assert not st.any() and not gh.any() and not hp.any(), f"slot {s} keeps key-derived bytes"


def _queue_stats(lib):
    f = lib.tlsrec__engine_queue_stats
    f.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    out = []
    for q in range(8):
        b, r = ctypes.c_uint64(), ctypes.c_uint64()
        assert f(q, ctypes.byref(b), ctypes.byref(r)) == 0
        out.append((b.value, r.value))
    assert f(8, None, None) == M.ERR_SSL_BAD_INPUT_DATA
    return out


def test_concurrent_cbc_and_gcm_callers_use_their_own_queues():
    """8 threads with a transform each, half CBC and half AES-GCM, 32 records each way: every
    result exact, and the CBC batches counted in the CBC queues, the GCM ones in the GCM queues"""
    lib = _abi.load()
    lib.tlsrec__server_enable(0)                    # the GCM calls through the coalescing launch path too
    q0 = _queue_stats(lib)
    errors = []
    per = 32

    def cbc_worker(tid):
        c = Conn(R.CIPHER_AES_128_CBC, R.MAC_SHA256, tid % 2, 500 + tid)
        try:
            for n in range(per):
                ln = (n * 389 + tid * 71) % 3000
                ctr = (n + 7 * tid).to_bytes(8, "big")
                pt = prng_bytes(tid * 1000 + n, ln)
                rec = M.Record(ctr=ctr, type=23, ver=TLS, buf=bytearray(16) + bytearray(pt) + bytearray(96),
                               data_offset=16, data_len=ln)
                st = c.t.encrypt_buf(rec)
                want = A.encrypt(c.enc, bytes(rec.buf[0:16]) + pt + bytes(96), 16, ln, ctr, 23, TLS)
                if (st, rec.data_offset, rec.data_len, bytes(rec.buf)) != (0, want.data_offset, want.data_len, want.buf):
                    errors.append((tid, n, "encrypt"))
                buf, off, dl, rtype = c.seal(pt, ctr)
                bad, rec = c.decrypt(buf, off, dl, ctr, rtype)
                if bad or rec.data() != pt:
                    errors.append((tid, n, "decrypt", bad))
        except Exception as e:          # noqa: BLE001 (reported below)
            errors.append((tid, "exception", repr(e)))
        finally:
            c.close()

    def gcm_worker(tid):
        key, iv = prng_bytes(3000 + tid, 16), prng_bytes(4000 + tid, 16)
        t = M.Transform(M.VERSION_TLS1_3, M.CIPHER_AES_128_GCM, key, key, iv, iv)
        ot = O.Transform(M.VERSION_TLS1_3, M.CIPHER_AES_128_GCM, key, key, iv, iv)
        try:
            for n in range(per):
                ln = (n * 389 + tid * 71) % 3000
                ctr = (n + 7 * tid).to_bytes(8, "big")
                pt = prng_bytes(tid * 1000 + n, ln)
                buf = bytearray(pt) + bytearray(64)
                rec = M.Record(ctr=ctr, type=23, ver=TLS, buf=buf, data_offset=0, data_len=ln)
                orec = O.Record(ctr=ctr, type=23, ver=TLS, buf=bytearray(buf), data_offset=0, data_len=ln)
                if t.encrypt_buf(rec) != 0 or ot.encrypt_buf(orec) != 0 or rec.data() != orec.data():
                    errors.append((tid, n, "gcm encrypt"))
                    continue
                if t.decrypt_buf(rec) != 0 or rec.data() != pt:
                    errors.append((tid, n, "gcm decrypt"))
        except Exception as e:          # noqa: BLE001 (reported below)
            errors.append((tid, "exception", repr(e)))
        finally:
            t.close()

    ths = [threading.Thread(target=cbc_worker if i % 2 else gcm_worker, args=(i,)) for i in range(8)]
    try:
        for th in ths:
            th.start()
        for th in ths:
            th.join(timeout=300)
    finally:
        lib.tlsrec__server_enable(1)
    assert not errors, errors[:5]
    d = [(b1 - b0, r1 - r0) for (b0, r0), (b1, r1) in zip(q0, _queue_stats(lib))]
    assert [r for _, r in d] == [4 * per, 4 * per, 0, 0, 0, 0, 4 * per, 4 * per], d
    assert all(b > 0 for b, _ in (d[0], d[1], d[6], d[7])), d
