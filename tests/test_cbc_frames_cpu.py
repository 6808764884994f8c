"""AES-CBC + HMAC connections in the stream and DTLS layers: everything that
needs no GPU.  The framing model of tests/cbc_frames_ref.py is pinned against
the oracle's C restatement (oracle/stream.c, oracle/dtls.c) by plugging the
oracle's AEAD transform into it; the host helpers tlsrec_*_out_size_cbc are
checked against the model's wire lengths; the new symbols and the layout of
tlsrec_frame_opts against include/tlsrec.h."""
from __future__ import annotations

import ctypes
import os
import re

import pytest

import mbedtls_amd as M
from mbedtls_amd import _abi
from mbedtls_amd import cbc as C
from mbedtls_amd import dtls as D
from mbedtls_amd import stream as S
import oracle as O
from tests import cbc_frames_ref as F
from tests import cbc_ref as R
from tests.prng import prng_bytes

MACS = [R.MAC_SHA1, R.MAC_SHA256, R.MAC_SHA384]
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tlsrec.h")


def ctr(epoch, seq):
    return epoch.to_bytes(2, "big") + (seq % (1 << 48)).to_bytes(6, "big")


def _aead(cipher, version, seed, cid=b"", gran=16):
    k, iv = prng_bytes(seed, O.KEYLEN[cipher]), prng_bytes(seed + 1, 12)
    t = O.Transform(version, cipher, k, k, iv, iv, granularity=gran)
    t.set_cid(cid, cid)
    head = 8 if (version == O.TLS1_2 and cipher != O.CHACHA20_POLY1305) else 0
    return t, F.OracleAead(t, head, cid)


AEADS = [(O.AES_128_GCM, O.TLS1_2), (O.AES_256_GCM, O.TLS1_3), (O.CHACHA20_POLY1305, O.TLS1_3),
         (O.CHACHA20_POLY1305, O.TLS1_2), (O.AES_256_CCM_8, O.TLS1_2)]


# ---- the framing model against the C restatement ---------------------------------
@pytest.mark.parametrize("cipher,version", AEADS)
def test_stream_model_matches_the_oracle(cipher, version):
    t, p = _aead(cipher, version, 100 + cipher, gran=32 if version == O.TLS1_3 else 16)
    for i, (n, frag, c0) in enumerate([(0, 100, 0), (1, 16384, 5), (300, 100, 1 << 40), (16385, 16384, 7),
                                        (40000, 4096, 9), (3000, 1000, (1 << 64) - 2)]):
        pt = prng_bytes(200 + i, n)
        want = O.stream_encrypt(t, pt, 23 if i % 2 else 22, c0.to_bytes(8, "big"), frag)
        assert F.stream_encrypt(p, pt, 23 if i % 2 else 22, c0.to_bytes(8, "big"), frag) == want, i
    _, w, _, _ = O.stream_encrypt(t, prng_bytes(9, 300), 23, bytes(8), 100)
    one = len(w) // 3

    def empty(k):
        buf = bytearray(64)
        rec = O.Record(ctr=k.to_bytes(8, "big"), type=23, ver=b"\x03\x03", buf=buf, data_offset=p.head, data_len=0)
        assert t.encrypt_buf(rec) == 0
        return bytes([23, 3, 3]) + rec.data_len.to_bytes(2, "big") + rec.data()

    cases = [(w, 0, 0), (w + w[:7], 0, 1), (w[:one] + bytes([24]) + w[one + 1:], 0, 0),       # bad type
             (w[:one] + w[one:one + 1] + b"\x03\x05" + w[one + 3:], 0, 0),                     # version
             (w[:one] + w[one:one + 3] + b"\x00\x00" + w[one + 5:], 0, 0),                     # zero length
             (w[:one] + w[one:one + 3] + b"\x40\x21" + w[one + 5:], 0, 0),                     # too long
             (w[:one + 20] + bytes([w[one + 20] ^ 0x80]) + w[one + 21:], 0, 0),                # bad MAC
             (w[:4], 0, 0), (b"", 0, 0), (w[:one + 9], 0, 0),                                  # partial records
             (bytes([20, 3, 3, 0, 1, 1]) + w, 0, 0),                                           # CCS first
             (b"".join(empty(k) for k in range(4)), 0, 0), (b"".join(empty(k) for k in range(2)), 0, 2),
             (empty((1 << 64) - 1), (1 << 64) - 1, 0)]                                         # counter wrap
    for i, (data, c0, nbz) in enumerate(cases):
        want = O.stream_decrypt(t, data, c0.to_bytes(8, "big"), nbz)
        got = F.stream_decrypt(p, data, c0.to_bytes(8, "big"), nbz)
        assert got == want, (i, got[0], want[0])


@pytest.mark.parametrize("cid", [b"", b"\xaa\xbb\xcc"], ids=["nocid", "cid"])
@pytest.mark.parametrize("cipher", [O.AES_128_GCM, O.CHACHA20_POLY1305, O.AES_256_CCM_8])
def test_dtls_model_matches_the_oracle(cipher, cid):
    t, p = _aead(cipher, O.TLS1_2, 300 + cipher, cid)
    t0, p0 = _aead(cipher, O.TLS1_2, 300 + cipher)                # the same key without a CID
    for i, (n, frag, c8) in enumerate([(0, 100, ctr(1, 0)), (1, 16384, ctr(2, 5)), (3000, 1200, ctr(1, 1 << 40)),
                                        (20000, 16384, ctr(3, 7)), (3000, 1000, ctr(4, (1 << 48) - 2))]):
        pt = prng_bytes(400 + i, n)
        want = O.dtls_encrypt(t, pt, 23 if i % 2 else 22, c8, frag)
        assert F.dtls_encrypt(p, pt, 23 if i % 2 else 22, c8, frag) == want, i

    def rec(seq, epoch=1, n=200, typ=23, tt=t):
        st, w, _, _ = O.dtls_encrypt(tt, prng_bytes(seq, n), typ, ctr(epoch, seq), 16384)
        assert st == 0
        return w

    def flip(w, at):
        return w[:at] + bytes([w[at] ^ 0x10]) + w[at + 1:]

    g = [rec(k) for k in range(12)]
    empty = [rec(40 + k, n=0) for k in range(5)]
    cl = len(cid)
    conns = [
        ({}, [g[0], g[0], rec(50, epoch=0), rec(60, epoch=2), flip(g[2], 40) + g[3], g[3],            # replays, epochs,
              b"\x17\xfe\xfd" + bytes(8), g[4] + b"\x40" + g[5][1:], g[5], g[2]]),                   # a dropped datagram
        ({}, [flip(g[6], 50), g[6], g[6]]),
        ({"badmac_limit": 2}, [g[0], flip(g[1], 30), g[2], flip(g[3], 30), g[4], g[5]]),
        ({"badmac_limit": 3, "badmac_seen": 1}, [flip(g[1], 30), g[2]]),
        ({}, [g[0] + b"\x17\xfe\xfd", g[1]]), ({}, [g[0], b"", g[1]]), ({}, [g[0][:20], g[1][:-1], g[2]]),
        ({"window_top": 9, "window": 0b1011}, [g[9], g[8], g[7], g[6], g[10]]),
        ({}, [rec(100), rec(30), rec(100), rec(37)]), ({"anti_replay": 0}, [g[3], g[3], g[1]]),
        ({}, [empty[0] + empty[1] + empty[2] + empty[3] + g[11], empty[4]]), ({"nb_zero": 2}, [empty[0], g[1]]),
        ({}, [rec(70, n=0, typ=22), g[1]]),
        ({}, [g[1][:1] + b"\xfe\xff" + g[1][3:], g[1][:1] + b"\x03\x03" + g[1][3:], g[1]]),
        ({"ignore_unexpected_cid": 1}, [rec(1), rec(2, tt=t0), rec(3)]), ({}, [rec(1), rec(2, tt=t0), rec(3)]),
        ({"cid_len": 0}, [rec(1)]),
        ({}, [g[0] + bytes(O.DTLS_MAX_DATAGRAM)]),
    ]
    for i, (stt, dgs) in enumerate(conns):
        so, sm = O.DtlsState(), F.DtlsState()
        for st in (so, sm):
            st.anti_replay, st.in_epoch, st.cid_len = 1, 1, cl
            for f, v in stt.items():
                setattr(st, f, v)
        want = O.dtls_decrypt(t, so, dgs)
        got = F.dtls_decrypt(p, sm, dgs)
        assert got == want, (i, got[0], want[0])
        assert (sm.window_top, sm.window, sm.badmac_seen, sm.nb_zero) == \
            (so.window_top, so.window, so.badmac_seen, so.nb_zero), i


def test_cbc_limits_are_the_header_arithmetic():
    """ssl_misc.h:283-400 with MAC_ADD 48 and PADDING_ADD 256 against the AEAD-only build's values"""
    a, c = F.limits(False), F.limits(True)
    assert (a.max_in_record, a.out_buf_space, a.dtls_max_datagram, a.dtls_out_buffer_len) == \
        (_abi.MAX_IN_RECORD, _abi.OUT_BUF_SPACE, _abi.DTLS_MAX_DATAGRAM, _abi.DTLS_OUT_BUFFER_LEN)
    assert (c.max_in_record, c.out_buf_space, c.dtls_max_datagram, c.dtls_out_buffer_len) == \
        (_abi.MAX_IN_RECORD_CBC, _abi.OUT_BUF_SPACE_CBC, _abi.DTLS_MAX_DATAGRAM_CBC, _abi.DTLS_OUT_BUFFER_LEN_CBC) == \
        (16709, 16704, 16765, 16765)
    src = open(HEADER).read()
    for name, v in (("MAX_IN_RECORD_CBC", 16709), ("OUT_BUF_SPACE_CBC", 16704), ("DTLS_MAX_DATAGRAM_CBC", 16765),
                    ("DTLS_OUT_BUFFER_LEN_CBC", 16765), ("FRAME_CBC", 1)):
        assert re.search(r"#define\s+TLSREC_%s\s+%du?\b" % (name, v), src), name


# ---- tlsrec_*_out_size_cbc ---------------------------------------------------------
def _key(mac, etm, cid=b""):
    return R.Key(R.CIPHER_AES_128_CBC, mac, etm, prng_bytes(1, 16), prng_bytes(2, R.MACLEN[mac]), cid)


@pytest.mark.parametrize("mac", MACS)
@pytest.mark.parametrize("etm", [0, 1])
def test_out_size_cbc_is_the_models_wire_length(mac, etm):
    """content lengths 0..80 and 16 383 / 16 384, max_frag 1 / 100 / 0; stream, DTLS without and with a CID.
    The wire length is that of the model's sealed records (the lengths below 400 bytes are sealed;
    above, wire_body -- the same arithmetic the sealed ones pin)."""
    for cid in (None, b"", b"\x01\x02\x03\x04\x05"):
        dtls = cid is not None
        p = F.CbcProtector(_key(mac, etm, cid or b""), lambda k: bytes(16))
        for frag in (1, 100, 0):
            for n in list(range(81)) + [16383, 16384]:
                got = D.out_size_cbc(mac, etm, len(cid), n, frag) if dtls else S.out_size_cbc(mac, etm, n, frag)
                assert got == F.out_size(p, n, frag, dtls), (cid, frag, n)
                if n <= 80 or frag == 0:
                    st, w, nrec, _ = (F.dtls_encrypt if dtls else F.stream_encrypt)(p, bytes(n), 23, bytes(8),
                                                                                   frag or 16384)
                    assert st == 0 and len(w) == got and nrec == (n + (frag or 16384) - 1) // (frag or 16384)
    # without a CID a record is tlsrec_cbc_record_len
    assert S.out_size_cbc(mac, etm, 1000, 0) == 5 + C.record_len(mac, etm, 1000)
    assert D.out_size_cbc(mac, etm, 0, 1000, 0) == 13 + C.record_len(mac, etm, 1000)


def test_out_size_cbc_unknown_ids():
    for mac, etm in ((0, 0), (4, 1), (R.MAC_SHA256, 2), (R.MAC_SHA256, -1)):
        assert S.out_size_cbc(mac, etm, 100) == 0 and D.out_size_cbc(mac, etm, 0, 100) == 0
    assert D.out_size_cbc(R.MAC_SHA1, 0, 33, 100) == 0              # cid_len > TLSREC_CID_LEN_MAX
    assert D.out_size_cbc(R.MAC_SHA1, 0, 32, 100) != 0


# ---- symbols and layout -------------------------------------------------------------
NEW = ["tlsrec_stream_decrypt_ex", "tlsrec_stream_encrypt_ex", "tlsrec_dtls_decrypt_ex", "tlsrec_dtls_encrypt_ex",
       "tlsrec_stream_out_size_cbc", "tlsrec_dtls_out_size_cbc"]


def test_new_symbols_are_exported_and_declared():
    L = M.load()
    src = open(HEADER).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in _abi.SIGNATURES
        assert re.search(r"\b%s\s*\(" % name, src), name


def test_frame_opts_layout_is_the_headers():
    src = open(HEADER).read()
    m = re.search(r"typedef struct tlsrec_frame_opts \{(.*?)\} tlsrec_frame_opts;", src, re.S)
    fields = re.findall(r"^\s*(const uint8_t \*|uint32_t )\s*(\w+);", m.group(1), re.M)
    assert [(t.strip(), n) for t, n in fields] == [("uint32_t", "flags"), ("uint32_t", "reserved"),
                                                   ("const uint8_t *", "cbc_ivs")]
    o = _abi.CFrameOpts
    assert [f[0] for f in o._fields_] == ["flags", "reserved", "cbc_ivs"]
    assert (o.flags.offset, o.reserved.offset, o.cbc_ivs.offset, ctypes.sizeof(o)) == (0, 4, 8, 16)
    x = S.frame_opts()
    assert (x.flags, x.reserved, x.cbc_ivs) == (_abi.FRAME_CBC, 0, None)


def test_bad_options_are_refused_before_the_table_is_touched():
    """unknown flag bits, reserved != 0, and a send call with TLSREC_FRAME_CBC and no IVs: BAD_INPUT_DATA"""
    L = M.load()
    E = M.ERR_SSL_BAD_INPUT_DATA
    for flags, reserved in ((2, 0), (_abi.FRAME_CBC | 0x80000000, 0), (_abi.FRAME_CBC, 1), (0, 7)):
        o = ctypes.byref(_abi.CFrameOpts(flags, reserved, None))
        assert L.tlsrec_stream_decrypt_ex(None, None, 0, None, None, None, 0, None, None, None, o) == E
        assert L.tlsrec_dtls_decrypt_ex(None, None, 0, None, 0, None, None, None, None, 0, None, None, None, o) == E
        assert L.tlsrec_stream_encrypt_ex(None, None, 0, None, None, None, None, 0, None, None, None, o) == E
        assert L.tlsrec_dtls_encrypt_ex(None, None, 0, None, None, None, None, 0, None, None, None, o) == E
    o = ctypes.byref(_abi.CFrameOpts(_abi.FRAME_CBC, 0, None))
    assert L.tlsrec_stream_encrypt_ex(None, None, 0, None, None, None, None, 0, None, None, None, o) == E
    assert L.tlsrec_dtls_encrypt_ex(None, None, 0, None, None, None, None, 0, None, None, None, o) == E
